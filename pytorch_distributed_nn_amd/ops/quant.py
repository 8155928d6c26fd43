"""Weight-only fp8 storage of the decode linears: OCP e4m3fn codes with one power-of-two scale per output row.

The definition both devices share (csrc/kernels/gemm_skinny_fp8.hip computes the same on the GPU).  For a weight ``w``
bf16 [N][K], row n: amax = max_k |w[n][k]|; e = the smallest integer with amax 2^-e <= 448, found exactly from
frexp(amax) = (m, x), m in [0.5, 1): e = x - 9 if m <= 0.875 else x - 8, clamped to [-100, 100], and 0 for amax == 0;
q[n][k] = e4m3fn(w[n][k] 2^-e) (round to nearest even; the product is exact and at most 448); inv[n] = 2^e (fp32).  The
dequantised weight dq[n][k] = value(q[n][k]) inv[n] is exactly a bf16 number, so a model whose decode weights are
replaced by dq is an ordinary bf16 model: the reference of the fp8 decode path.  Non-finite weights are outside the
contract."""
from __future__ import annotations

import torch

E4M3 = torch.float8_e4m3fn


def quantize_rows_reference(w):
    """w [N][K] (bf16, or any float dtype holding bf16 values) -> (q uint8 [N][K] e4m3fn codes, inv fp32 [N])"""
    wf = w.detach().float()
    m, x = torch.frexp(wf.abs().amax(dim=1))
    e = torch.where(m <= 0.875, x - 9, x - 8).clamp(-100, 100)
    e = torch.where(m == 0, torch.zeros_like(e), e)
    q = torch.ldexp(wf, -e[:, None]).to(E4M3).view(torch.uint8)
    return q, torch.ldexp(torch.ones_like(m), e)


def dequantize_rows(q, inv, dtype=torch.bfloat16):
    """(q, inv) -> dq [N][K]: exact in bf16"""
    return (q.view(E4M3).float() * inv[:, None].float()).to(dtype)
