"""Fused GPT-2 building blocks (BASELINE.json config 4: "GPT-2-small transformer DDP bf16 8xMI355X
(LayerNorm + attention GEMM HIP kernels)").  The reference has no transformer (SURVEY.md §2 lists CNNs and
MLPs only), so this is new capability exercising the same engine: every GEMM runs on the MFMA engine of
``csrc/kernels/gemm_mfma.hip`` and every row op on ``csrc/kernels/transformer.hip``.

A whole pre-LN block ``x + attn(ln_1(x))`` -> ``+ mlp(ln_2(.))`` is ONE autograd Function
(:class:`GPT2BlockFn`) so the backward schedules its own kernels (fused epilogues, no autograd glue):

forward                                              backward
  ln1 = LN(x)                 layernorm_fwd            dh   = dx2 . Wfc2 * gelu'(u)   gemm_nt_ex (w_kn, dgelu epilogue)
  qkv = ln1 Wqkv^T + b        gemm_nt_ex(bias)         dWfc2 += dx2^T h ; dbfc2 = colsum(dx2)
  S   = Q K^T (per b, h)      gemm_batched(causal=1)   dln2 = dh . Wfc ; dWfc, dbfc
  P   = softmax(S/sqrt(d))    attn_softmax_fwd         dx1  = LN2_bwd(dln2) + dx2     (residual fused)
  y   = P V                   gemm_batched(causal=2)   dy   = dx1 . Wproj ; dWproj, dbproj
  x1  = x + y Wproj^T + b     gemm_nt_ex(res=x)        attention bwd (dV, dP, dS, dQ, dK: 4 batched GEMMs
  ln2 = LN(x1)                                               + attn_softmax_bwd), written into dqkv
  h   = gelu(ln2 Wfc^T + b)   gemm_nt_ex(GELU, aux=u)  dln1 = dqkv . Wqkv ; dWqkv, dbqkv
  x2  = x1 + h Wfc2^T + b     gemm_nt_ex(res=x1)       dx   = LN1_bwd(dln1) + dx1

The residual stream is bf16 [B*T][D]; LayerNorm statistics, GEMM accumulation, softmax and all weight
gradients are fp32.  Attention (head dim 64, T % 128 == 0) runs the fused flash kernels of
``csrc/kernels/attention.hip`` (scores never leave registers; backward recomputes P from the saved
log-sum-exp); other shapes fall back to the materialised path below (batched MFMA GEMMs with causal tile
skipping + row-softmax kernels).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

from ..optim.flat import direct_grad, grad_ready
from . import linear as BL
from . import kernels as K
from .side_stream import GradSink, side_stream
from .. import tuning as _tuning

BF16 = torch.bfloat16
F32 = torch.float32


# ------------------------------------------------------------------------------------------------
# attention core on a packed qkv [B*T][3D] bf16 tensor
# ------------------------------------------------------------------------------------------------
def attention_fwd(qkv, B, T, H, causal=True):
    """-> y [B*T][D] bf16, P [B*H*T][T] bf16 (saved for backward)."""
    D = qkv.shape[1] // 3
    d = D // H
    ld = 3 * D
    dev = qkv.device
    S = torch.empty(B * H * T, T, device=dev, dtype=F32)
    P = torch.empty(B * H * T, T, device=dev, dtype=BF16)
    lse = torch.empty(B * H * T, device=dev, dtype=F32)
    y = torch.empty(B * T, D, device=dev, dtype=BF16)
    q, k, v = qkv, qkv[:, D:], qkv[:, 2 * D:]
    # S[b,h] = Q K^T : A = Q [T][d] (K-major), B = K [T][d] (K-major)
    K.gemm_batched(q, ld, (T * ld, d), 0, k, ld, (T * ld, d), 0, S, T, (H * T * T, T * T), T, T, d, (B, H),
                   causal=1 if causal else 0)
    K.attn_softmax_fwd(S, P, lse, B * H * T, T, 1.0 / math.sqrt(d), causal)
    # y[b, :, h] = P V : A = P [T][T], B = V stored [T(k)][d]
    K.gemm_batched(P, T, (H * T * T, T * T), 0, v, ld, (T * ld, d), 1, y, D, (T * D, d), T, d, T, (B, H),
                   causal=2 if causal else 0)
    return y, P, S


def attention_bwd(dy, qkv, P, B, T, H, causal=True, dS_buf=None):
    """dy [B*T][D] -> dqkv [B*T][3D].  ``dS_buf``: fp32 [B*H*T][T] scratch (the forward's S)."""
    D = qkv.shape[1] // 3
    d = D // H
    ld = 3 * D
    dev = qkv.device
    dqkv = torch.empty(B * T, ld, device=dev, dtype=BF16)
    q, k, v = qkv, qkv[:, D:], qkv[:, 2 * D:]
    dq, dk, dv = dqkv, dqkv[:, D:], dqkv[:, 2 * D:]
    sP = (H * T * T, T * T)
    # dV = P^T dO : A = P stored [q][k] = [K][M] (amode 1), B = dO stored [q][d] = [K][N] (bmode 1)
    K.gemm_batched(P, T, sP, 1, dy, D, (T * D, d), 1, dv, ld, (T * ld, d), T, d, T, (B, H),
                   causal=3 if causal else 0)
    # dP = dO V^T (fp32)
    dP = dS_buf if dS_buf is not None else torch.empty(B * H * T, T, device=dev, dtype=F32)
    K.gemm_batched(dy, D, (T * D, d), 0, v, ld, (T * ld, d), 0, dP, T, sP, T, T, d, (B, H),
                   causal=1 if causal else 0)
    # dS = P * (dP - rowsum(P dP)) / sqrt(d), written over P (row-local, read-before-write per element)
    dS = P
    K.attn_softmax_bwd(P, dP, dS, B * H * T, T, 1.0 / math.sqrt(d), causal)
    # dQ = dS K : B = K stored [k][d] = [K][N]
    K.gemm_batched(dS, T, sP, 0, k, ld, (T * ld, d), 1, dq, ld, (T * ld, d), T, d, T, (B, H),
                   causal=2 if causal else 0)
    # dK = dS^T Q : A = dS stored [q][k] = [K][M], B = Q stored [q][d] = [K][N]
    K.gemm_batched(dS, T, sP, 1, q, ld, (T * ld, d), 1, dk, ld, (T * ld, d), T, d, T, (B, H),
                   causal=3 if causal else 0)
    return dqkv


def use_flash(T, D, H):
    return D // H == 64 and T % 128 == 0


def attention_reference(qkv, B, T, H, causal=True, mask=None):
    """fp32 PyTorch reference of :func:`attention_fwd` (tests, CPU path).  ``mask``: optional bool [B][T][T] (or
    broadcastable to [B][H][T][T]), True where the query (row) sees the key (column); it replaces ``causal``
    (:func:`doc_visible` builds the causal packed-document one)."""
    D = qkv.shape[1] // 3
    q, k, v = qkv.float().view(B, T, 3, H, D // H).permute(2, 0, 3, 1, 4)
    if mask is not None:
        m = mask if mask.dim() == 4 else mask.unsqueeze(1)
        y = F.scaled_dot_product_attention(q, k, v, attn_mask=m)
    else:
        y = F.scaled_dot_product_attention(q, k, v, is_causal=causal)
    return y.transpose(1, 2).reshape(B * T, D)


def doc_bounds_reference(idx, eot):
    """PyTorch form of kernels.doc_bounds (any device): idx [B][T] -> (doc_start, doc_end) int32 [B][T].  Token t starts
    a document iff t == 0 or token t - 1 is ``eot``: the EOT token belongs to the document it ends."""
    B, T = idx.shape
    t = torch.arange(T, device=idx.device).expand(B, T)
    is_eot = idx == eot
    starts = torch.zeros_like(is_eot)
    starts[:, 1:] = is_eot[:, :-1]
    ds = torch.where(starts, t, torch.zeros_like(t)).cummax(1).values
    ends = torch.where(is_eot, t + 1, torch.full_like(t, T))
    de = ends.flip(1).cummin(1).values.flip(1)
    return ds.to(torch.int32).contiguous(), de.to(torch.int32).contiguous()


def doc_visible(doc_start):
    """bool [B][T][T] of the causal packed-document mask: query q sees key k iff doc_start[b][q] <= k <= q"""
    B, T = doc_start.shape
    i = torch.arange(T, device=doc_start.device)
    return (i[None, None, :] <= i[None, :, None]) & (i[None, None, :] >= doc_start.long()[:, :, None])


# ------------------------------------------------------------------------------------------------
# dropout: the counter-based generator of csrc/kernels/dropout_rng.h in torch integers (any device), and the
# (seed, step) state of a model
# ------------------------------------------------------------------------------------------------
SITE_EMBD = 0x7fffffff      # site = 4 * layer + {0 attention probabilities, 1 attention residual, 2 MLP residual}
_M32, _M64 = (1 << 32) - 1, (1 << 64) - 1


def dropout_threshold(p):
    """p in [0, 1) -> thr in [0, 255]: an element is kept iff its byte >= thr, p_eff = thr / 256"""
    p32 = torch.tensor(float(p), dtype=F32).item()
    if not 0.0 <= p32 < 1.0:
        raise ValueError(f"dropout: p must be in [0, 1), got {p!r}")
    return min(255, int(p32 * 256.0 + 0.5))


def dropout_p_eff(p):
    return dropout_threshold(p) / 256.0


def dropout_scale(p):
    return 256.0 / (256 - dropout_threshold(p))


def _mix64(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _drop_key(seed, step, site, stream):
    z = _mix64(((seed & _M64) + 0x9E3779B97F4A7C15 * ((step & _M64) + 1)) & _M64)
    z = _mix64(z ^ ((site << 32) | stream))
    return z & _M32, z >> 32


def _mul32(x, c):
    """x * c mod 2^32 on an int64 tensor holding 32-bit values, without leaving 63 bits"""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & _M32


def _drop_words(k0, k1, idx):
    x = (idx + k0) & _M32
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7feb352d)
    x = x ^ (x >> 15)
    x = (x + k1) & _M32
    x = _mul32(x, 0x846ca68b)
    return x ^ (x >> 16)


def dropout_keep_reference(state, site, p, rows=None, attn=None, device="cpu"):
    """The keep bits of the dropout kernels (bool): ``rows`` = (R, D) -> [R][D] for a row op, ``attn`` = (B, H, T) ->
    [B][H][T(q)][T(k)] for the attention probabilities.  ``state`` = the int64 (seed, step) tensor, or the pair."""
    seed, step = (int(v) for v in (state.tolist() if torch.is_tensor(state) else state))
    thr = dropout_threshold(p)
    sh = 8 * torch.arange(4, device=device)

    def bits(k, n, shape):
        w = _drop_words(k[0], k[1], torch.arange(n, device=device, dtype=torch.int64))
        return (((w[:, None] >> sh) & 255) >= thr).reshape(shape)

    if rows is not None:
        R, D = rows
        return bits(_drop_key(seed, step, site, 0), R * (D // 4), (R, D))
    B, H, T = attn
    return torch.stack([bits(_drop_key(seed, step, site, s), T * (T // 4), (T, T)) for s in range(B * H)]).view(B, H, T, T)


def dropout_seed():
    """torch's initial seed folded with the rank, so ranks draw different masks; kept inside int64"""
    import torch.distributed as dist
    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    return (torch.initial_seed() + 0x9E3779B97F4A7C15 * rank) & ((1 << 63) - 1)


def dropout_advance(state):
    """One training forward: -> a fresh snapshot of (seed, step) for this forward's Functions (and their backward, so
    that a forward run in between does not change its masks); ``state`` then counts one step further.  Two
    stream-ordered device ops, captured with the step: a replay reads and advances the live state."""
    snap = state.clone()
    state[1:].add_(1)
    return snap


# ------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, weight, bias, eps):
        y, mean, rstd = K.layernorm_fwd(x2, weight, bias, eps)
        ctx.save_for_backward(x2, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x2, weight, mean, rstd = ctx.saved_tensors
        dx, dg, db = K.layernorm_bwd(gy.to(BF16), x2, weight, mean, rstd)
        return dx, dg, db, None


def layer_norm(x, weight, bias, eps=1e-5):
    if not x.is_cuda:
        return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)
    shp = x.shape
    x2 = x.reshape(-1, shp[-1]).to(BF16).contiguous()
    return _LayerNorm.apply(x2, weight, bias, eps).view(shp)


# ------------------------------------------------------------------------------------------------
# embedding (token + position)
# ------------------------------------------------------------------------------------------------
class EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, T, wte_k, wpe_k, wte, wpe, head_direct=False, tail=None, drop=None):
        ctx.save_for_backward(idx)
        ctx.conf = (T, wte_k.shape, wpe.shape)
        ctx.wpe, ctx.wte = wpe, wte
        ctx.head_direct = head_direct       # the tied LM head accumulates its wte gradient in the arena too
        ctx.tail = tail                     # (ddp, wte): split tied embedding, wte is NOT an input (wte=None)
        ctx.drop = drop                     # (p, state snapshot): dropout on wte + wpe
        x = K.embedding_fwd(idx, wte_k, wpe_k, T)
        if drop is not None:
            K.dropout_add_fwd(x, None, drop[0], drop[1], SITE_EMBD, out=x)
        return x

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        T, s_te, s_pe = ctx.conf
        if ctx.drop is not None:            # the rows both tables receive are the masked ones
            g = K.dropout_bwd(g, ctx.drop[0], ctx.drop[1], SITE_EMBD)
        if ctx.tail is not None:
            # split tied embedding (parallel/ddp.py reduce_sparse_rows): the LM head's dense gradient was announced
            # (and its bucket all-reduced) at the start of the backward; these B*T rows are gathered from every rank
            # and added on top after it
            ddp, wte = ctx.tail
            ctx.tail = None
            tpe = direct_grad(ctx.wpe)
            dwpe = tpe if tpe is not None else torch.zeros(s_pe, device=g.device, dtype=F32)
            K.embedding_bwd(idx, g, None, dwpe, T)
            if tpe is not None:
                grad_ready(ctx.wpe)
                dwpe = None
            gw = wte.grad
            ddp.reduce_sparse_rows(wte, idx, g, lambda i, r, sc: K.embedding_bwd(i, r, gw, None, T, scale=sc))
            ctx.wpe = ctx.wte = None
            return None, None, None, None, None, dwpe, None, None, None
        # wte is tied with the LM head, whose backward ran first and (with a flat arena) already accumulated
        # its part in place: the embedding adds its rows on top (atomics) and announces the parameter, so no
        # zero-filled temporaries and no autograd sum of the two gradients
        tte = direct_grad(ctx.wte) if ctx.head_direct else None
        dwte = tte if tte is not None else torch.zeros(s_te, device=g.device, dtype=F32)
        tpe = direct_grad(ctx.wpe)
        dwpe = tpe if tpe is not None else torch.zeros(s_pe, device=g.device, dtype=F32)
        K.embedding_bwd(idx, g, dwte, dwpe, T)
        if tpe is not None:
            grad_ready(ctx.wpe)
            dwpe = None
        if tte is not None:
            grad_ready(ctx.wte)
            dwte = None
        ctx.wpe = ctx.wte = None
        return None, None, None, None, dwte, dwpe, None, None, None


# ------------------------------------------------------------------------------------------------
# one transformer block
# ------------------------------------------------------------------------------------------------
def _wgrad(g, x, shape):
    dw = torch.zeros(shape, device=g.device, dtype=F32)
    BL.wgrad_acc(g, x, dw)
    return dw


class _Sink(GradSink):
    """Routes parameter gradients straight into the flat arena when possible (optim.flat.direct_grad):
    the GEMM / column-sum / LayerNorm kernels accumulate in place, the op returns None for the parameter
    and announces it with grad_ready.  Otherwise the gradient is returned to autograd.

    tuning gpt2_side_wgrad: arena-bound weight gradients run on the ResNets' weight-gradient side stream
    (ops/side_stream.py) beside the data-gradient chain, joined like theirs (GradSink.done)."""

    def linear(self, p_w, p_b, g, x):
        tw = self.target(p_w)
        tb = self.target(p_b) if p_b is not None else None
        bias_in = tb if _tuning.get("bias_in_wgrad") else None
        side = side_stream(g.device) if (tw is not None and (p_b is None or tb is not None)
                                         and _tuning.get("gpt2_side_wgrad") and g.is_cuda) else None
        if side is not None:
            self.side = side
            self.fork(torch.cuda.current_stream(g.device))
            with torch.cuda.stream(side):
                bias_done = BL.wgrad_acc(g, x, tw, bias=bias_in, plan_cus=_tuning.get("wgrad_plan_cus"))
                if p_b is not None and not bias_done:
                    K.colsum(g, out=tb, accumulate=True, deterministic=not _tuning.get("colsum_atomic"))
            for t in (g, x):
                t.record_stream(side)
            return None, None
        bias_done = False
        if tw is not None:
            # the bias gradient fused into the weight-gradient GEMM when both land in the arena
            bias_done = BL.wgrad_acc(g, x, tw, bias=bias_in)
            rw = None
        else:
            rw = _wgrad(g, x, p_w.shape)
        rb = None
        if p_b is not None and not bias_done:
            if tb is not None:
                K.colsum(g, out=tb, accumulate=True, deterministic=not _tuning.get("colsum_atomic"))
            else:
                rb = K.colsum(g)
        return rw, rb

    def layernorm(self, dy, x, w, m, r, dres, p_w, p_b):
        acc = self.acc(p_w, p_b)
        if acc is not None:
            dx, _, _ = K.layernorm_bwd(dy, x, w, m, r, dres=dres, acc=tuple(acc))
            return dx, None, None
        return K.layernorm_bwd(dy, x, w, m, r, dres=dres)


class BlockConf(NamedTuple):
    """What one block needs besides tensors and parameters; a plain tuple of the first four fields or more serves too
    (``BlockConf(*t)``)."""
    B: int
    T: int
    H: int
    eps: float
    metas: object = None        # the block's fp8 metas: the forward GEMMs run on the fp8 engine
    doc: object = None          # (doc_start, doc_end) int32 [B][T]: packed-document mask
    drop: object = None         # (attn_pdrop, resid_pdrop, state snapshot, layer) of a training forward with dropout


_NO_DROP = (0.0, 0.0, None, 0)


class _BlockAttn:
    """The attention of one block on its packed qkv [B*T][3D]: the flash kernels where they apply (:func:`use_flash`),
    else the materialised chain, which has neither a document mask nor dropout and refuses both."""

    def __init__(self, conf, D):
        self.B, self.T, self.H = B, T, H = conf[:3]
        self.flash = use_flash(T, D, H)
        self.scale = 1.0 / math.sqrt(D // H)
        self.doc = conf.doc
        p_attn, _, dstate, layer = conf.drop or _NO_DROP
        # the probabilities never leave the kernel's registers: the mask is drawn inside it, at site 4 * layer
        self.drop = (p_attn, dstate, 4 * layer) if p_attn > 0 else None
        if self.doc is not None and not self.flash:
            raise ValueError(f"packed-document attention needs the fused kernels (head dim 64, T % 128 == 0); got head "
                             f"dim {D // H}, T = {T}: the unfused attention chain has no document mask")
        if self.drop is not None and not self.flash:
            raise ValueError(f"attention dropout needs the fused kernels (head dim 64, T % 128 == 0); got head dim "
                             f"{D // H}, T = {T}: the unfused attention chain has no dropout (attn_pdrop = 0 runs it)")

    def fwd(self, qkv):
        """-> y, P, S: P is lse2 and S None on the flash kernels; the chain's S is the backward's fp32 dP scratch"""
        if self.flash:
            return (*K.flash_attn_fwd(qkv, self.B, self.T, self.H, self.scale, doc=self.doc, drop=self.drop), None)
        return attention_fwd(qkv, self.B, self.T, self.H)

    def bwd(self, qkv, y, dy, P, S):
        if self.flash:
            return K.flash_attn_bwd(qkv, y, dy, P, self.B, self.T, self.H, self.scale, doc=self.doc, drop=self.drop)
        return attention_bwd(dy, qkv, P, self.B, self.T, self.H, dS_buf=S)


class GPT2BlockFn(torch.autograd.Function):
    """params: ln1_w, ln1_b, attn_w, attn_b, proj_w, proj_b, ln2_w, ln2_b, fc_w, fc_b, fc2_w, fc2_b
    shadows: bf16 copies of attn_w [3D][D], proj_w [D][D], fc_w [4D][D], fc2_w [D][4D].  conf: :class:`BlockConf`."""

    @staticmethod
    def forward(ctx, x, conf, shadows, *params):
        conf = BlockConf(*conf)
        eps, metas = conf.eps, conf.metas
        _, p_res, dstate, layer = conf.drop or _NO_DROP
        attn = _BlockAttn(conf, x.shape[1])
        ln1w, ln1b, _, attn_b, _, proj_b, ln2w, ln2b, _, fc_b, _, fc2_b = params
        wqkv, wproj, wfc, wfc2 = shadows
        if metas is not None:
            from .fp8 import linear_fp8_fwd

            def lin(inp, i, wk, **kw):      # forward GEMM on the fp8 engine (weights: params[2/4/8/10])
                return linear_fp8_fwd(inp, params[i], metas[(i - 2) // 2 if i < 6 else (i - 4) // 2], **kw)
        else:
            def lin(inp, i, wk, **kw):
                return BL.linear_fwd(inp, wk, **kw)
        ln1, m1, r1 = K.layernorm_fwd(x, ln1w, ln1b, eps)
        qkv = lin(ln1, 2, wqkv, bias=attn_b)
        y, P, S = attn.fwd(qkv)
        if p_res > 0:       # the branch output is dropped before the add: GEMM with bias only, then one row pass
            x1 = lin(y, 4, wproj, bias=proj_b)
            K.dropout_add_fwd(x1, x, p_res, dstate, 4 * layer + 1, out=x1)
        else:
            x1 = lin(y, 4, wproj, bias=proj_b, res=x)
        ln2, m2, r2 = K.layernorm_fwd(x1, ln2w, ln2b, eps)
        u = torch.empty(x.shape[0], wfc.shape[0], device=x.device, dtype=BF16)
        h = lin(ln2, 8, wfc, bias=fc_b, act=2, aux=u)
        if p_res > 0:
            x2 = lin(h, 10, wfc2, bias=fc2_b)
            K.dropout_add_fwd(x2, x1, p_res, dstate, 4 * layer + 2, out=x2)
        else:
            x2 = lin(h, 10, wfc2, bias=fc2_b, res=x1)
        ctx.save_for_backward(x, ln1, m1, r1, qkv, P, y, x1, ln2, m2, r2, u, h, ln1w, ln2w, *shadows)
        ctx.conf = conf
        ctx.attn = attn
        ctx.S = S          # materialised path: reused as the fp32 dP scratch in backward
        ctx.params = params
        return x2

    @staticmethod
    def backward(ctx, g):
        (x, ln1, m1, r1, qkv, P, y, x1, ln2, m2, r2, u, h, ln1w, ln2w, wqkv, wproj, wfc, wfc2) = ctx.saved_tensors
        Pm = ctx.params
        ctx.params = None
        sink = _Sink()
        g = g.contiguous()
        if g.is_cuda and _tuning.get("wt_layer_batch"):
            # the four data-gradient GEMMs' transposed weights of this block in one launch, just before use
            from .functional import prefetch_weight_t
            prefetch_weight_t((Pm[10], Pm[8], Pm[4], Pm[2]))
        _, p_res, dstate, layer = ctx.conf.drop or _NO_DROP
        # MLP (resid_pdrop: the branch sees the masked gradient, the residual path -- LN2's dres -- the whole one)
        gm = K.dropout_bwd(g, p_res, dstate, 4 * layer + 2) if p_res > 0 else g
        du = BL.linear_dgrad(gm, wfc2, dgelu=u, p=Pm[10])                      # (g . Wfc2) * gelu'(u)
        dfc2_w, dfc2_b = sink.linear(Pm[10], Pm[11], gm, h)
        dln2 = BL.linear_dgrad(du, wfc, p=Pm[8])
        dfc_w, dfc_b = sink.linear(Pm[8], Pm[9], du, ln2)
        dx1, dln2w, dln2b = sink.layernorm(dln2, x1, ln2w, m2, r2, g, Pm[6], Pm[7])
        # attention
        dm = K.dropout_bwd(dx1, p_res, dstate, 4 * layer + 1) if p_res > 0 else dx1
        dy = BL.linear_dgrad(dm, wproj, p=Pm[4])
        dproj_w, dproj_b = sink.linear(Pm[4], Pm[5], dm, y)
        dqkv = ctx.attn.bwd(qkv, y, dy, P, ctx.S)
        ctx.S = None
        dln1 = BL.linear_dgrad(dqkv, wqkv, p=Pm[2])
        dattn_w, dattn_b = sink.linear(Pm[2], Pm[3], dqkv, ln1)
        dx, dln1w, dln1b = sink.layernorm(dln1, x, ln1w, m1, r1, dx1, Pm[0], Pm[1])
        sink.done()
        return (dx, None, None, dln1w, dln1b, dattn_w, dattn_b, dproj_w, dproj_b, dln2w, dln2b, dfc_w, dfc_b,
                dfc2_w, dfc2_b)


# ------------------------------------------------------------------------------------------------
# inference: key/value cache, prefill and decode-step blocks (plain functions, no autograd)
# ------------------------------------------------------------------------------------------------
class KVCache:
    """The key/value cache of one generation batch on the GPU (csrc/kernels/attention_decode.hip): one K and one V
    allocation bf16 [L][B][H][Tmax][64], ``lens`` int32 [B] on the device (tokens of sequence b already cached; the
    decode kernels read it there, the host never does) and the fp32 scratch of the split decode kernel, sized for ``S``
    queries per sequence (S > 1: :func:`block_step`).  Slots at or past lens[b] may hold anything, so :meth:`reset`
    only zeroes ``lens``."""

    def __init__(self, model, B, Tmax, device, chunk=None, S=1):
        c = model.config
        need_fused_kernels(c.n_embd, c.n_head)
        if B < 1 or Tmax < 1:
            raise ValueError(f"KVCache: B = {B}, Tmax = {Tmax}")
        if not (isinstance(S, int) and 1 <= S <= K.DECODE_MAX_S):
            raise ValueError(f"KVCache: 1 <= S <= {K.DECODE_MAX_S}, got S = {S!r}")
        self.B, self.H, self.Tmax, self.L, self.S = B, c.n_head, Tmax, c.n_layer, S
        self.chunk = K.DECODE_CHUNK if chunk is None else chunk
        self.k = torch.zeros(c.n_layer, B, c.n_head, Tmax, 64, device=device, dtype=BF16)
        self.v = torch.zeros_like(self.k)
        self.lens = torch.zeros(B, device=device, dtype=torch.int32)
        self.part = torch.empty(K.attn_decode_multi_ws(B, S, c.n_head, Tmax, self.chunk), device=device, dtype=F32)

    def reset(self):
        self.lens.zero_()

    def truncate(self, lens):
        """Rewind: lens[b] = min(lens[b], ``lens``[b]) on the device (``lens``: an int, or B of them).  Slots past lens
        may hold anything, so rewinding is only that."""
        self.lens.copy_(torch.minimum(self.lens, torch.as_tensor(lens, device=self.lens.device).to(torch.int32)
                                      .expand_as(self.lens)))


def need_fused_kernels(D, H, T=None):
    """Generation runs on the head-dim-64 kernels only, a prefill (``T`` given) on the flash kernels (:func:`use_flash`)"""
    hd = D // H
    if hd == 64 and D % H == 0 and (T is None or T % 128 == 0):
        return
    if T is not None:
        raise ValueError(f"generation needs the fused kernels (head dim 64, T % 128 == 0); got head dim {hd}, T = {T}")
    raise ValueError(f"generation needs the fused kernels (head dim 64); got head dim {hd}: the decode attention kernel "
                     f"has no other head dim (the CPU path runs any)")


def _block_infer(x, eps, shadows, params, lin, attn, *args, **kw):
    """The forward kernel sequence of :class:`GPT2BlockFn` with nothing saved, x bf16 [rows][D] -> x2: ``lin`` is the
    linear of the four GEMMs, ``attn(qkv, *args, **kw)`` takes the packed qkv to the attention output."""
    ln1w, ln1b, _, attn_b, _, proj_b, ln2w, ln2b, _, fc_b, _, fc2_b = params
    wqkv, wproj, wfc, wfc2 = shadows
    ln1, _, _ = K.layernorm_fwd(x, ln1w, ln1b, eps)
    y = attn(lin(ln1, wqkv, bias=attn_b), *args, **kw)
    x1 = lin(y, wproj, bias=proj_b, res=x)
    ln2, _, _ = K.layernorm_fwd(x1, ln2w, ln2b, eps)
    h = lin(ln2, wfc, bias=fc_b, act=2)
    return lin(h, wfc2, bias=fc2_b, res=x1)


def block_prefill(x, conf, shadows, params, cache, layer):
    """One block over the whole (padded) prompt: x bf16 [B*T][D], conf = (B, T, H, eps) or a :class:`BlockConf`,
    T % 128 == 0 -> x2; the K and V of every position also go into slots 0..T-1 of ``cache`` layer ``layer``.  The
    linears are bf16 (BL.linear_fwd) whatever config.fp8 says."""
    B, T, H, eps = conf[:4]
    need_fused_kernels(x.shape[1], H, T)

    def attn(qkv):      # a prompt is one document, and nothing is dropped
        K.kv_cache_fill(qkv, cache.k[layer], cache.v[layer], B, T)
        return K.flash_attn_fwd(qkv, B, T, H, 1.0 / math.sqrt(x.shape[1] // H))[0]
    return _block_infer(x, eps, shadows, params, BL.linear_fwd, attn)


def block_step(x, conf, shadows, params, cache, layer, S=1):
    """One block on the S new tokens per sequence: x bf16 [B*S][D] -> x2, row b*S + j at position cache.lens[b] + j; the
    decode attention also stores the new k, v rows.  No host read-back; cache.lens unchanged.  S == 1, a decode step:
    BL.linear_fwd_decode and K.attn_decode.  S > 1, a speculative verify step: K.attn_decode_multi, and K.gemm_skinny
    for every M = B*S <= K.SKINNY_ROWS, whose row bits do not depend on M: a row gets the bits of the S == 1 step."""
    B, _, H, eps = conf[:4]
    if S == 1:
        lin, attn, multi = BL.linear_fwd_decode, K.attn_decode, {}
    else:
        if S > cache.S or x.shape[0] != B * S or x.shape[0] > K.SKINNY_ROWS:    # (the text of block_verify, now this S > 1)
            raise ValueError(f"block_verify: {x.shape[0]} rows for B = {B}, S = {S} (cache S = {cache.S}, at most "
                             f"{K.SKINNY_ROWS} rows)")
        lin, attn, multi = K.gemm_skinny, K.attn_decode_multi, {"S": S}
    return _block_infer(x, eps, shadows, params, lin, attn, cache.k[layer], cache.v[layer], cache.lens, chunk=cache.chunk,
                        part=cache.part, scale=1.0 / math.sqrt(x.shape[1] // H), **multi)


def block_extend(x, conf, shadows, params, cache, layer):
    """One block on Tq new tokens per sequence behind a non-empty cache: x bf16 [B*Tq][D], conf = (B, Tq, H, eps), Tq a
    multiple of K.EXTEND_TILE -> x2, row b*Tq + j at position cache.lens[b] + j.  The attention appends the new k, v rows
    to ``cache`` layer ``layer`` and then runs K.attn_extend over the cache; the linears are BL.linear_fwd.  No host
    read-back; cache.lens unchanged."""
    B, Tq, H, eps = conf[:4]
    need_fused_kernels(x.shape[1], H)
    if Tq % K.EXTEND_TILE or x.shape[0] != B * Tq or cache.B != B:
        raise ValueError(f"block_extend: {x.shape[0]} rows for B = {B}, Tq = {Tq} (a multiple of {K.EXTEND_TILE}), cache "
                         f"B = {cache.B}")

    def attn(qkv):
        K.kv_cache_append(qkv, cache.k[layer], cache.v[layer], cache.lens)
        return K.attn_extend(qkv, cache.k[layer], cache.v[layer], cache.lens, scale=1.0 / math.sqrt(x.shape[1] // H))
    return _block_infer(x, eps, shadows, params, BL.linear_fwd, attn)


# ------------------------------------------------------------------------------------------------
# final LayerNorm + tied LM head + cross-entropy
# ------------------------------------------------------------------------------------------------
class LMHeadLossFn(torch.autograd.Function):
    """loss = mean CE(LN_f(x) . Wte^T, targets); logits bf16 [B*T][V] live only inside this op.  ``label_smoothing``
    and ``z_loss`` select the smoothed / z-regularised loss of the same kernels (ops/kernels.py xent_fwd)."""

    @staticmethod
    def forward(ctx, x, targets, eps, wte_k, lnw, lnb, wte, head_direct=False, split=False, training=False,
                label_smoothing=0.0, z_loss=0.0):
        ctx.ls = (label_smoothing, z_loss)
        ctx.head_direct = head_direct
        ctx.split = split                   # split tied embedding: the head announces wte itself
        xf, m, r = K.layernorm_fwd(x, lnw, lnb, eps)
        logits = BL.linear_fwd(xf, wte_k)
        # training (grad mode on at the call): the forward also writes the unscaled gradient softmax - onehot over
        # the logits (one read + one write of the 8192 x 50304 logits instead of three passes); the backward then
        # scales the head's 8192 x 768 products by grad_out / count instead of the logits gradient
        ctx.fused = training and _tuning.get("xent_fused") and logits.is_cuda and K.xent_fwd_grad_ok(logits)
        if ctx.fused:
            _, lse, acc, _ = K.xent_fwd_grad(logits, targets, label_smoothing=label_smoothing, z_loss=z_loss)
        else:
            _, lse, acc = K.xent_fwd(logits, targets, label_smoothing=label_smoothing, z_loss=z_loss)
        ctx.save_for_backward(x, xf, m, r, logits, targets, lse, acc, lnw, wte_k)
        ctx.eps = eps
        ctx.params = (lnw, lnb)
        ctx.wte = wte
        return acc[0] / acc[1].clamp_min(1.0)

    @staticmethod
    def backward(ctx, g):
        x, xf, m, r, logits, targets, lse, acc, lnw, wte_k = ctx.saved_tensors
        gs = g.reshape(1)
        if gs.dtype != torch.float32:
            gs = gs.float()
        if ctx.fused:           # logits hold the unscaled gradient: scale the products instead (device scalar, no sync)
            dlogits = logits
            sc = gs / acc[1:2].clamp_min(1.0)
            dxf = BL.linear_dgrad(dlogits, wte_k, p=ctx.wte)
            dxf.mul_(sc)
            xf = xf.clone()
            xf.mul_(sc)
        else:
            dlogits = K.xent_bwd(logits, targets, lse, gs, 1.0, count=acc[1:2], label_smoothing=ctx.ls[0],
                                 z_loss=ctx.ls[1])
            dxf = BL.linear_dgrad(dlogits, wte_k, p=ctx.wte)
        tte = direct_grad(ctx.wte) if ctx.head_direct else None
        if tte is not None:     # tied weight: the embedding backward adds its part and announces it
            BL.wgrad_acc(dlogits, xf, tte)
            dwte = None
            if ctx.split:       # ... unless its rows are reduced separately: the dense part is complete now
                grad_ready(ctx.wte)
        else:
            dwte = _wgrad(dlogits, xf, wte_k.shape)     # summed with the embedding's by autograd
        sink = _Sink()
        dx, dlnw, dlnb = sink.layernorm(dxf, x, lnw, m, r, None, *ctx.params)
        ctx.params = None
        ctx.wte = None
        sink.done()
        return dx, None, None, None, dlnw, dlnb, dwte, None, None, None, None, None
