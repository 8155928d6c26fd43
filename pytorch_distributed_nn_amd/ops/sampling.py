"""The token draw of csrc/kernels/sample.hip in plain torch: ``sample_reference`` implements the definition in that file's
header line for line (weights in fp64, the generator of csrc/kernels/dropout_rng.h in Python integers), runs on any
device, and is what ``GPT2.generate(sampler="device")`` uses on the CPU.  It is the documented meaning of the kernel;
the kernel's 64-bit fixed-point weights agree with it to about 2^-19 of the row's total weight.

Temperature and top_p are fp32 values (as the kernel receives them): both are rounded to fp32 first."""
import struct

import torch

SITE_SAMPLE = 0x7ffffffe
_M64 = (1 << 64) - 1


def _mix64(z):
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & _M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & _M64
    return z ^ (z >> 31)


def uniform(seed, step, stream):
    """u of (seed, step, stream): the top 24 bits of word 0 of the stream's key, times 2^-24"""
    z = _mix64((int(seed) + 0x9E3779B97F4A7C15 * (int(step) + 1)) & _M64)
    z = _mix64(z ^ ((SITE_SAMPLE << 32) | (int(stream) & 0xffffffff)))
    k0, k1 = z & 0xffffffff, z >> 32
    x = k0                                                    # granule 0
    x ^= x >> 16
    x = x * 0x7feb352d & 0xffffffff
    x ^= x >> 15
    x = (x + k1) & 0xffffffff
    x = x * 0x846ca68b & 0xffffffff
    x ^= x >> 16
    return (x >> 8) * 2.0 ** -24


def _f32(v):
    return struct.unpack("f", struct.pack("f", float(v)))[0]


def sample_row(row, temperature, top_k, top_p, u):
    """one row -> (token, thr, nkeep); ``row`` a 1-D tensor, ``u`` a float in [0, 1), or a 1-D float64 tensor of them
    (then ``token`` is an int64 tensor: the row drawn once per u)"""
    l = row.double()
    l = torch.where(torch.isnan(l), torch.full_like(l, float("-inf")), l)
    V = l.numel()
    ninf = float("-inf")
    m = l.max().item()
    many = torch.is_tensor(u)

    def out(token, thr, nkeep):
        return (torch.full_like(u, token, dtype=torch.int64) if many else token), thr, nkeep
    if m == ninf:
        return out(0, ninf, 0)
    T = _f32(temperature)
    if T == 0.0:
        return out(int((l == m).nonzero()[0]), m, 1)
    thr = ninf
    if top_k is not None and int(top_k) < V:
        thr = torch.topk(l, int(top_k)).values[-1].item()
    kept = l >= thr
    w = torch.where(kept & (l > ninf), torch.exp((l - m) / T), torch.zeros_like(l))
    p = None if top_p is None else _f32(top_p)
    if p is not None and 0.0 < p < 1.0:
        vals, inv = torch.unique(l[kept], return_inverse=True)                  # ascending
        mass = torch.zeros_like(vals).index_add_(0, inv, w[kept])
        above = mass.flip(0).cumsum(0).flip(0)                                  # sum of w over l_i >= vals[j]
        ok = (above >= p * w.sum()).nonzero()
        thr = max(thr, vals[int(ok[-1]) if ok.numel() else vals.numel() - 1].item())
    S = l >= thr
    w = w * S
    c = w.cumsum(0)
    # the first i with c[i] > u W (never an element of weight 0: the one before it has the same sum); none: the fallback
    us = u.to(dtype=torch.float64, device=l.device) if many else torch.tensor([float(u)], dtype=torch.float64, device=l.device)
    token = torch.searchsorted(c, us * c[-1], right=True).clamp(max=int((w > 0).nonzero()[-1]))
    return (token if many else int(token[0])), thr, int(S.sum())


def sample_reference(logits, temperature=1.0, top_k=None, top_p=None, *, state=None, u=None, eos_token=None,
                     finished=None):
    """logits [B][V] (any float dtype, any device) -> (tok int64 [B], thr fp32 [B], nkeep int32 [B]).  Row b draws with
    u = uniform(seed, step, b) for ``state`` = (seed, step) (a pair of ints or an int64 [2] tensor), or with ``u[b]``
    when ``u`` is given.  With ``eos_token``, ``finished`` (bool or uint8 [B]) is read and updated in place."""
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"sample_reference: logits must be [B][V], got {tuple(logits.shape)}")
    if not float(temperature) >= 0.0:
        raise ValueError(f"sample_reference: temperature must be >= 0, got {temperature!r}")
    if top_k is not None and int(top_k) < 1:
        raise ValueError(f"sample_reference: top_k must be >= 1, got {top_k!r}")
    if top_p is not None and not float(top_p) > 0.0:
        raise ValueError(f"sample_reference: top_p must be > 0, got {top_p!r}")
    if (eos_token is None) != (finished is None) and eos_token is not None:
        raise ValueError("sample_reference: eos_token needs finished")
    B = logits.shape[0]
    if u is None:
        if state is None:
            raise ValueError("sample_reference: state = (seed, step) or u is required")
        seed, step = (int(v) for v in (state.tolist() if torch.is_tensor(state) else state))
        us = [uniform(seed, step, b) for b in range(B)]
    else:
        us = [min(max(int(float(v) * 2 ** 24), 0), 2 ** 24 - 1) * 2.0 ** -24 if v == v else 0.0
              for v in (u.tolist() if torch.is_tensor(u) else u)]
    fin = finished.tolist() if finished is not None else [0] * B
    toks, thrs, nks = [], [], []
    for b in range(B):
        if eos_token is not None and fin[b]:
            t, th, nk = int(eos_token), 0.0, 0
        else:
            t, th, nk = sample_row(logits[b], temperature, top_k, top_p, us[b])
        toks.append(t)
        thrs.append(th)
        nks.append(nk)
    dev = logits.device
    tok = torch.tensor(toks, dtype=torch.int64, device=dev)
    if eos_token is not None:
        finished |= (tok == int(eos_token)).to(finished.dtype)
    return tok, torch.tensor(thrs, dtype=torch.float32, device=dev), torch.tensor(nks, dtype=torch.int32, device=dev)
