"""Weight-only fp8 storage of the decode linears: OCP e4m3fn codes with one power-of-two scale per output row.

The definition both devices share (csrc/kernels/gemm_skinny_fp8.hip computes the same on the GPU).  For a weight ``w``
bf16 [N][K], row n: amax = max_k |w[n][k]|; e = the smallest integer with amax 2^-e <= 448, found exactly from
frexp(amax) = (m, x), m in [0.5, 1): e = x - 9 if m <= 0.875 else x - 8, clamped to [-100, 100], and 0 for amax == 0;
q[n][k] = e4m3fn(w[n][k] 2^-e) (round to nearest even; the product is exact and at most 448); inv[n] = 2^e (fp32).  The
dequantised weight dq[n][k] = value(q[n][k]) inv[n] is exactly a bf16 number, so a model whose decode weights are
replaced by dq is an ordinary bf16 model: the reference of the fp8 decode path.  Non-finite weights are outside the
contract.

Weight-only MXFP4 storage (``decode_weights="mxfp4"``; csrc/kernels/gemm_skinny_fp4.hip computes the same on the GPU):
OCP microscaling fp4, e2m1 codes with one e8m0 scale per block of 32 consecutive reduction elements.  For a weight ``w``
bf16 [N][K], K % 32 == 0, row n and block j: amax = max |w[n][32 j .. 32 j + 31]|; e = the smallest integer with amax 2^-e
<= 6, from frexp(amax) = (m, x): e = x - 3 if m <= 0.75 else x - 2, clamped to [-100, 100], 0 for amax == 0; sc[n][j] =
e + 127 (uint8).  q = e2m1(w 2^-e): the sign bit of w, two exponent bits, one mantissa bit; the magnitudes 0, 0.5, 1, 1.5,
2, 3, 4, 6 are the codes 0 .. 7; round to nearest, ties to the even code (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 -> 0, 1, 1, 2,
2, 4, 4); the product is exact and at most 6.  Two codes per byte, element 2 i in the low nibble of byte i: q uint8
[N][K / 2].  dq[n][k] = value(q[n][k]) 2^e[n][k / 32] is exactly a bf16 number, and |dq - w| <= max(2^-2 |w|, 2^-2 2^e).
Non-finite weights and blocks that would need |e| > 100 are outside the contract.

The stored forms are named, so that the two cannot be confused: :class:`Fp8Rows` (q, inv) and :class:`Mxfp4Blocks` (q, sc);
a plain pair is read as fp8, as before the second format."""
from __future__ import annotations

from collections import namedtuple

import torch

E4M3 = torch.float8_e4m3fn
Fp8Rows = namedtuple("Fp8Rows", "q inv")
Mxfp4Blocks = namedtuple("Mxfp4Blocks", "q sc")
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


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


def quantize_blocks_reference(w):
    """w [N][K] (bf16, or any float dtype holding bf16 values), K % 32 == 0 -> (q uint8 [N][K / 2] e2m1 codes, sc uint8
    [N][K / 32] e8m0 scales)"""
    wf = w.detach().float()
    N, K = wf.shape
    blk = wf.view(N, K // 32, 32)
    m, x = torch.frexp(blk.abs().amax(dim=2))
    e = torch.where(m <= 0.75, x - 3, x - 2).clamp(-100, 100)
    e = torch.where(m == 0, torch.zeros_like(e), e)
    a = torch.ldexp(blk, -e[..., None]).abs()                  # exact, <= 6; the comparisons are the rounding: ties to even
    ties = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)              # below an even code: the tie stays down; below an odd one: up
    mag = sum(((a > t) if i % 2 == 0 else (a >= t)).to(torch.uint8) for i, t in enumerate(ties))
    code = (mag | torch.signbit(blk).to(torch.uint8) << 3).view(N, K // 2, 2)
    return code[..., 0] | code[..., 1] << 4, (e + 127).to(torch.uint8)


def dequantize_blocks(q, sc, dtype=torch.bfloat16):
    """(q, sc) -> dq [N][K]: exact in bf16"""
    N, K = q.shape[0], 2 * q.shape[1]
    mag = torch.tensor(E2M1_VALUES, device=q.device)
    code = torch.stack([q & 15, q >> 4], dim=2).view(N, K // 32, 32).long()
    val = torch.where(code >= 8, -mag[code & 7], mag[code & 7])
    scale = torch.ldexp(torch.ones_like(sc, dtype=torch.float32), sc.int() - 127)
    return (val * scale[..., None]).view(N, K).to(dtype)
