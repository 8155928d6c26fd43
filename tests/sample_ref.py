"""A numpy float64 reference of the token draw defined in the header of csrc/kernels/sample.hip, the acceptance rule the
sampling kernel is held to, and the case list.  Shared by test_sample_ref_cpu.py, test_sample_gpu.py and
test_gpt2_generate_device_sampler_gpu.py.  The generator is tests/dropout_ref.py's (key, words) at site SITE_SAMPLE,
stream = row, granule 0: u = (word >> 8) * 2^-24.

For a row, ``analyse`` returns the exact top-k threshold t_k (decided on the raw values), the top-p threshold t_p with a
flag ``ambiguous`` when some candidate threshold's mass lies within EPS W_k of p W_k (then every threshold between the
first whose mass reaches p W_k - EPS W_k and the first whose mass reaches p W_k + EPS W_k is accepted), and, for a final
threshold, the set S and the normalised fp64 CDF C over it.  A token j is accepted for u iff j is in S and
C[j - 1] - EPS <= u <= C[j] + EPS (C[j - 1]: the sum before j).  The tokens this accepts around u carry at most
p_j + 2 EPS of probability mass, so a kernel with a wrong order, stream, temperature or set fails almost surely.

EPS = 2^-16.  Derivation: for a weight that matters ((m - l_i) / T <~ 20) the kernel forms the exponent argument
(l_i - m) log2(e) / T in fp32: |argument| <= 29, so its rounding errors (the subtraction, the product, the quotient
log2(e) / T) total about 29 * 3 * 2^-24 ~ 2^-17.6 absolute, a relative weight error of ln 2 times that ~ 2^-18.1, plus
a 1-ulp exp2 (2^-23) and the truncation to 2^-40 fixed point (2^-24 of W in total): about 2^-18 .. 2^-19 per weight,
which is also the error of any normalised partial sum (the sums themselves are exact integers).  x 8 is the margin for
the implementer's choice of fixed-point width or summation tree.  Worst observed distance / EPS on an MI355X over
cases() in both dtypes and over the gpt2_tiny generate test: 0.0 (WORST_OBSERVED: every u lay inside its token's fp64
interval; the tests print the figure of every run).  27 of the 892 top-p rows of cases() are ambiguous (3.0 %).
"""
import numpy as np
import torch

import dropout_ref as DRP

EPS = 2.0 ** -16
SITE_SAMPLE = 0x7ffffffe
NINF = float("-inf")
WORST_OBSERVED = 0.0           # distance / EPS of the worst accepted token over cases(), both dtypes

VS = [1, 7, 64, 1000, 4099, 50257, 50304, 65536]
BS = [1, 3, 8, 33]
PS = [None, 1e-6, 0.5, 0.9, 0.999, 1.0]
TS = [0.0, 0.05, 0.7, 1.0, 4.0]
FAMILIES = ["gauss1", "gauss8", "bf16_ties", "equal", "one_finite", "ninf_blocks", "nan", "offset_pos", "offset_neg"]
STATE = (20241020, 5)


def ks_of(V):
    return [None, 1, 2, 50, V, V + 5]


def uniform(seed, step, stream):
    k = DRP.key(seed, step, SITE_SAMPLE, stream)
    return float(int(DRP.words(k, np.zeros(1, dtype=np.uint32))[0]) >> 8) * 2.0 ** -24


def bf16_round(a):
    """float32 array -> the float32 values of its bf16 rounding"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


def make(family, B, V, seed):
    """float32 [B][V]"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, V)).astype(np.float32)
    if family == "gauss8":
        x *= 8
    elif family == "bf16_ties":
        x = bf16_round(np.round(x * 4) / 4 + (g.integers(0, 3, (B, V)) * 2.0 ** -6).astype(np.float32))
    elif family == "equal":
        x[:] = 1.5
    elif family == "one_finite":
        keep = g.integers(0, V, B)
        y = np.full_like(x, NINF)
        y[np.arange(B), keep] = x[np.arange(B), keep]
        x = y
    elif family == "ninf_blocks":
        for s in range(0, V, 2048):
            x[:, s:s + 1024] = NINF                     # whole 1024-element spans
        if V > 8:
            x[:, V - V // 5:] = NINF                    # and the row's tail
        x[:, V // 2] = 0.25                              # a finite value survives at every V
    elif family == "nan":
        x[g.random((B, V)) < 0.1] = np.nan
    elif family == "offset_pos":
        x += np.float32(3e4)
    elif family == "offset_neg":
        x -= np.float32(3e4)
    return x


def cases():
    """(family, B, V, k, p, T, seed): the product of the lists above pruned to 216 cases, 27 a vocabulary size.  The
    indices come from the case counter n with strides that do not alias: k and p walk all 36 pairs every 36 cases, T
    and B shift by one every cycle of theirs.  test_sample_ref_cpu.py asserts that every value of every list occurs."""
    out = []
    for n in range(len(VS) * len(FAMILIES) * 3):
        V, fam = VS[n // 27], FAMILIES[(n // 3) % 9]
        B = BS[(n + n // 4) % 4]
        if V > 5000:
            B = min(B, 3)
        elif V > 1000:
            B = min(B, 8)
        out.append((fam, B, V, ks_of(V)[n % 6], PS[(n + n // 6) % 6], TS[(n + n // 5) % 5], 1000 + n))
    return out


def analyse(row, T, k, p):
    """row float32 [V] -> dict: kind ('degenerate' | 'greedy' | 'draw'), l (float64, NaN -> -inf), m, tk, tp, thrs (the
    accepted final thresholds), ambiguous, token (degenerate and greedy only)"""
    l = row.astype(np.float64)
    l[np.isnan(l)] = NINF
    V, m = l.size, l.max()
    r = dict(l=l, m=m, V=V, ambiguous=False, top_p=False)
    if m == NINF:
        return dict(r, kind="degenerate", token=0, thrs=[NINF], nkeep=0)
    T = float(np.float32(T))
    if T == 0.0:
        return dict(r, kind="greedy", token=int(np.argmax(l == m)), thrs=[m], nkeep=1)
    tk = NINF
    if k is not None and k < V:
        tk = np.partition(l, V - k)[V - k]
    kept = l >= tk
    w = np.where(kept & (l > NINF), np.exp((l - m) / T), 0.0)
    r.update(kind="draw", T=T, tk=tk, w=w, thrs=[tk])
    p32 = None if p is None else float(np.float32(p))
    if p32 is not None and 0.0 < p32 < 1.0:
        sel = kept & (l > NINF)
        order = np.argsort(-l[sel], kind="stable")
        ls, cum = l[sel][order], np.cumsum(w[sel][order])
        last = np.r_[ls[1:] != ls[:-1], True]
        vals, mass = ls[last], cum[last]                        # descending values, the weight of everything >= each
        Wk = cum[-1]
        tgt = p32 * Wk

        def first(x):
            hit = np.nonzero(mass >= x)[0]
            return int(hit[0]) if hit.size else len(vals) - 1
        i0, ilo, ihi = first(tgt), first(tgt - EPS * Wk), first(tgt + EPS * Wk)
        amb = bool(np.any(np.abs(mass - tgt) <= EPS * Wk))
        r.update(tp=vals[i0], top_p=True, ambiguous=amb, thrs=[max(tk, v) for v in (vals[ilo:ihi + 1] if amb else [vals[i0]])])
    return r


def final_set(r, thr):
    """(S bool [V], C float64 [V]: the inclusive normalised CDF over S in index order) for the final threshold thr"""
    S = r["l"] >= thr
    w = r["w"] * S
    c = np.cumsum(w)
    return S, c / c[-1]


def accept(r, thr, token, u):
    """(ok, distance / EPS): distance of u from [C[j - 1], C[j]], 0 inside"""
    S, C = final_set(r, thr)
    if not (0 <= token < r["V"]) or not S[token]:
        return False, float("inf")
    lo = C[token - 1] if token else 0.0
    d = max(lo - u, u - C[token], 0.0)
    return d <= EPS, d / EPS


def check_row(row, T, k, p, u, token, thr=None, nkeep=None):
    """Assert the kernel's (token, thr, nkeep) of one row against the reference; thr / nkeep None (the caller cannot see
    the kernel's threshold): the token must be accepted under one of the accepted thresholds, of which an ambiguous
    row has more than one.  Returns distance / EPS."""
    r = analyse(row, T, k, p)
    if r["kind"] != "draw":
        assert token == r["token"], (r["kind"], token, r["token"])
        if thr is not None:
            assert nkeep == r["nkeep"] and (thr == r["thrs"][0]), (r["kind"], thr, nkeep, r["thrs"], r["nkeep"])
        return 0.0
    if thr is None:
        got = [accept(r, t, token, u) for t in r["thrs"]]
        assert any(ok for ok, _ in got), f"token {token} rejected for u = {u} under {r['thrs'][:4]} (T {T}, k {k}, p {p})"
        return min(d for ok, d in got if ok)
    else:
        assert any(thr == t for t in r["thrs"]), f"threshold {thr} not among the accepted {r['thrs'][:4]} (tk {r['tk']})"
        assert nkeep == int((r["l"] >= thr).sum()), (nkeep, int((r["l"] >= thr).sum()))
    ok, d = accept(r, thr, token, u)
    assert ok, f"token {token} rejected for u = {u}: distance {d:.3f} EPS (T {T}, k {k}, p {p}, thr {thr})"
    return d
