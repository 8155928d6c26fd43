// Weight-only MXFP4 decode: the block quantiser and the skinny-M GEMM that streams its codes.
//     y[M][N] = act(x[M][K] . dq[N][K]^T + bias[N]) (+ res[M][N]),   1 <= M <= 64,
// x, res, y bf16, fp32 accumulation, and the weight stored in the OCP microscaling fp4 format: e2m1 codes q[N][K / 2]
// (two per byte) with one e8m0 scale per 32 consecutive reduction elements, sc[N][K / 32]: 4.25 bits per weight against
// the 8 of gemm_skinny_fp8.hip and the 16 of gemm_skinny.hip.
//
// The format (pdnn_quant_blocks_mxfp4; ops/quant.py quantize_blocks_reference is the same definition in torch).  For row
// n and block j of 32 elements: amax = max |w[n][32 j .. 32 j + 31]|; e = the smallest integer with amax 2^-e <= 6, i.e.
// with frexp(amax) = (m, x), m in [0.5, 1): e = x - 3 if m <= 0.75 else x - 2, clamped to [-100, 100], 0 for amax == 0;
// sc[n][j] = e + 127.  q = e2m1(w 2^-e): a sign bit (the sign bit of w), two exponent bits, one mantissa bit; the
// magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 are the codes 0 .. 7; round to nearest, ties to the even code (0.25, 0.75, 1.25,
// 1.75, 2.5, 3.5, 5 -> 0, 1, 1, 2, 2, 4, 4); the product is exact and never above 6.  Element 2 i is the low nibble of
// byte i.  dq[n][k] = value(q[n][k]) 2^e[n][k / 32] is exactly a bf16 number: the GEMM below is an ordinary bf16 GEMM on
// dq.  |dq - w| <= max(2^-2 |w|, 2^-2 2^e).
// The quantiser runs one thread per block (w is contiguous, so block t of the whole tensor is elements [32 t, 32 t + 32),
// bytes [16 t, 16 t + 16) of q and byte t of sc): four 16-byte loads, every element read once for every K, the amax of the
// bf16 magnitudes as integers, the exponent rule on the bf16 exponent and mantissa fields, and the rounding in plain
// arithmetic, seven comparisons against the tie points, so that the ties are the definition's whatever the hardware's
// quantising conversion does with them (it was not measured against them).
//
// MFMA orientation, as gemm_skinny.hip: v_mfma_f32_16x16x32_bf16 with 16 weight rows as the A operand and 16 rows of x
// as the B operand, D[n][m]: lane l holds D[n = 4 (l >> 4) + j][m = l & 15].  MT in {1, 2, 4} (compile time) row tiles of
// x; rows >= M read row M - 1 again (clamped addresses): those columns of D are never stored.
//
// Stream and reduction permutation.  The reduction unit is 256 elements, one 128-byte line of a weight row: lane
// (r = l & 15, g = l >> 4) owns weight row n0 + r and bytes [32 g, 32 g + 32) of the line, two nontemporal 16-byte loads
// straight to VGPRs; the four lanes of a row cover the whole line.  A load is 32 elements = exactly one scale block, so
// a load's conversion has one scale: dword p (0..3) of load h (0, 1) is the A operand of one MFMA, the lane's elements
// [64 g + 32 h + 8 p, + 8) of the unit, four v_cvt_scalef32_pk_bf16_fp4 (two codes each, the block's scale as the fp32
// operand (byte) << 23: a power of two, so the result is exactly dq), and the x fragment is read from x's row at the
// same element offsets.
// Scales.  The two scale bytes of a lane's two loads of a unit are neighbours, sc[row][unit * 8 + 2 g + {0, 1}]: one
// 2-byte load per lane and unit, issued with the unit's weight loads, a step ahead of the conversions that use it.  Rows
// of sc are 2-byte aligned only for K % 64 == 0 (and an even base); otherwise (K % 64 == 32, wave-uniform) the two bytes
// are two byte loads.  For K % 64 == 0 every slice ends on a multiple of 64, so the two loads of a lane are inside the
// slice together.
//
// x traffic.  Per weight byte this kernel reads four times the x bytes of gemm_skinny.hip.  RG in {1, 2} (compile time)
// groups of 16 weight rows per wave share one x fragment: RG = 2 halves the x reads and the blocks and doubles a wave's
// weight bytes in flight; the accumulation order of a row does not depend on RG, so the bits do not.  skinny4_groups is
// the rule of (N, K, MT); profiles/gemm_skinny_fp4.txt has both.  At M > 32 (MT = 4, one group, no x ring) the kernel is
// bound by its x reads and conversions per MFMA and loses to both siblings (LM head, M = 64: 76 us against 52 fp8 and 58
// bf16); up to 16 rows it is the fastest of the three on every GPT-2 shape measured.
//
// Bytes in flight.  A wave keeps two steps of weights in registers, the one the MFMAs read and the next in flight; a
// step is two units (4 loads and 2 scale loads per lane and row group: 4 KiB per wave and 16 rows).  The GPT-2 shapes give
// a wave one or two units in all (the partition below), so a deeper ring would stay empty.  x runs one load (four MFMAs)
// ahead in a two-entry ring at MT <= 2; MT = 4 keeps one entry.
// Resource usage (the compiler's kernel-resource-usage report, gfx950; VGPRs + AGPRs at NW <= 4, VGPRs at NW = 6, 8; no
// spills, no scratch in any instantiation; LDS NW x RG x MT KiB):
//     MT = 1, RG = 1:  122 + 12, 127     3 waves / SIMD (NW <= 4), 4 (NW = 6, 8)
//     MT = 1, RG = 2:  146 + 24, 158     2, 3
//     MT = 2, RG = 1:  149 + 24, 161     2, 3
//     MT = 2, RG = 2:  180 + 48, 216     2, 2
//     MT = 4, RG = 1:  201 + 36, 226     2, 2
// MT = 4 with RG = 2 compiles to 256 VGPRs with spills at NW >= 6 (with one unit per step still 8 spilled registers) and
// one wave per SIMD below: it is not built, M > 32 runs one row group.  The quantiser: 50 VGPRs, 8 waves / SIMD.
//
// Partition of K, a function of (N, K) only (pdnn_gemm_skinny_fp4_plan).  A block has NW in {2, 3, 4, 6, 8} waves; wave
// v reduces the slice [v SL, min((v + 1) SL, K)), SL = ceil(units / NW) * 256, MFMA after MFMA in ascending order into
// one fp32 accumulator per row tile and row group; an empty slice contributes zeros.  NW is the smallest count that
// gives cdiv(N, 16) NW >= 1024 waves and divides the units of K, else the smallest with >= 1024 waves and NW <= units,
// else the largest NW <= units that divides them, else the largest NW <= units, else 2.  The NW partial tiles go through
// LDS and are added in wave order by wave i % NW for tile i, which applies the epilogue of gemm_skinny.hip: v = acc;
// v += bias; GELU (gelu_tanh) of the bf16-rounded v; v += res; round to nearest even.  No atomics, nothing depends on M,
// MT or RG: row b of an M-row call has the bits of the 1-row call on that row.
//
// Edges: the last groups when N % (16 RG) != 0 (weight rows clamped to N - 1, their columns never stored), the K tail
// (K % 32 == 0: a weight load, its scale and the four x loads that match it, past the slice's end are issued at offset
// 0 of the row; the codes are replaced by +0, which the x values there multiply to zero: a non-finite activation in
// x[m][0 .. 31] makes row m's whole output non-finite, as in the siblings) and rows >= M.  No access leaves q[N][K / 2],
// sc[N][K / 32], x[M][K] (+ ldx), [M][N] (+ ldc).
#include "gemm_common.h"

namespace {
using pg::gelu_tanh;

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

constexpr int S4_UNIT = 256;        // reduction elements of one load pair = eight MFMAs
constexpr int S4_MIN_WAVES = 1024;  // waves the grid should reach at 16 rows per wave (4 per CU)

// ------------------------------------------------------------------------------------------------ quantiser
__global__ void __launch_bounds__(256) quant_blocks_mxfp4_kernel(const bf16_t* __restrict__ w, long nblk,
                                                                 uint8_t* __restrict__ q, uint8_t* __restrict__ sc) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nblk) return;
    u16x8_t v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const u16x8_t*>(w + t * 32 + 8 * i);
    unsigned a = 0;                 // the magnitudes order as their bit patterns
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) a = max(a, (unsigned)(v[i][j] & 0x7FFF));
    int e = 0;
    if (a) {        // frexp: m = (1 + mant / 128) / 2, x = E - 126; m <= 0.75 <=> mant <= 64; a subnormal clamps to -100
        e = (int)(a >> 7) - 126 - ((a & 127) <= 64 ? 3 : 2);
        e = min(max(e, -100), 100);
    }
    const float s = __uint_as_float((unsigned)(127 - e) << 23);
    u32x4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned d = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float m = fabsf(bf2f(v[i][j]) * s);       // exact, <= 6
            const unsigned c = (unsigned)(m > 0.25f) + (m >= 0.75f) + (m > 1.25f) + (m >= 1.75f) + (m > 2.5f) + (m >= 3.5f) +
                               (m > 5.f);
            d |= (c | (unsigned)(v[i][j] >> 15) << 3) << (4 * j);
        }
        o[i] = d;
    }
    *reinterpret_cast<u32x4_t*>(q + t * 16) = o;
    sc[t] = (uint8_t)(e + 127);
}

// ------------------------------------------------------------------------------------------------ GEMM
// waves per block for (N, K); the slice of a wave is then ceil(units / NW) * 256
int skinny4_plan(int N, int K) {
    const long groups = cdiv(N, 16), units = cdiv(K, S4_UNIT);
    const int cands[5] = {2, 3, 4, 6, 8};
    for (int c : cands)
        if (groups * c >= S4_MIN_WAVES && units % c == 0) return c;
    for (int c : cands)
        if (groups * c >= S4_MIN_WAVES && c <= units) return c;
    for (int i = 4; i >= 0; --i)
        if (cands[i] <= units && units % cands[i] == 0) return cands[i];
    for (int i = 4; i >= 0; --i)
        if (cands[i] <= units) return cands[i];
    return 2;
}

// row groups per wave for (N, K, MT): two where the halved grid still gives every SIMD a wave, which of the GPT-2 shapes
// is the LM head.  Measured (profiles/gemm_skinny_fp4.txt, section 1, us at M = 1 / 8 / 16, one | two groups): LM head
// K = 768 8.95 / 11.33 / 16.78 | 9.32 / 10.60 / 12.89, K = 1024 11.23 / 14.77 / 21.71 | 11.53 / 13.75 / 17.36; the block
// linears lose 0.2 - 2.3 us with two groups (half the blocks on a grid that is already short of waves)
int skinny4_groups(int N, int K, int MT) {
    return MT < 4 && cdiv(N, 32) * skinny4_plan(N, K) >= S4_MIN_WAVES ? 2 : 1;
}

// 8 e2m1 codes (one dword) of a weight row -> 8 bf16 of dq, exact: sc = 2^e of the codes' block
typedef __bf16 s4_bf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x8_t cvt8(unsigned a, float sc) {
    const s4_bf2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 1);
    const s4_bf2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 3);
    const u32x4_t o = {__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1), __builtin_bit_cast(unsigned, p2),
                       __builtin_bit_cast(unsigned, p3)};
    return __builtin_bit_cast(u16x8_t, o);
}

template <int RG, int NU>
struct S4W {
    u32x4_t v[RG][2 * NU];      // load i: unit i >> 1, elements [64 g + 32 (i & 1), + 32) of it
    unsigned s[RG][NU];         // unit u: the scale bytes of its two loads, load h in bits [8 h, 8 h + 8)
};
template <int MT>
struct S4X {
    u16x8_t v[MT][4];           // one load's worth: piece p = elements [64 g + 32 h + 8 p, + 8), the B operand of MFMA p
};

template <int MT, int NW, int RG>
__global__ void __launch_bounds__(NW * 64) gemm_skinny_fp4_kernel(const bf16_t* __restrict__ x, long ldx,
                                                                  const uint8_t* __restrict__ q,
                                                                  const uint8_t* __restrict__ sc, bf16_t* __restrict__ out,
                                                                  long ldc, int M, int N, int K, int SL, int pair,
                                                                  const float* __restrict__ bias, int act,
                                                                  const bf16_t* __restrict__ res) {
    constexpr int NU = 2;                       // units per step
    constexpr int STEP = NU * S4_UNIT;
    __shared__ __attribute__((aligned(16))) f32x4_t red[NW][RG * MT][64];
    // the wave index through readfirstlane: the compiler then knows that k0, k1 and every branch on them are wave-uniform
    // (scalar branches in place of EXEC-predicated regions around the MFMAs, and 6 - 8 fewer VGPRs)
    const int tid = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * (16 * RG);
    const int k0 = min(wv * SL, K), k1 = min(k0 + SL, K);
    const uint8_t* qrow[RG];                    // lane r owns weight rows n0 + 16 c + r
    const uint8_t* srow[RG];
#pragma unroll
    for (int c = 0; c < RG; ++c) {
        const long row = min(n0 + 16 * c + r, N - 1);
        qrow[c] = q + row * (K >> 1);
        srow[c] = sc + row * (K >> 5);
    }
    const bf16_t* xrow[MT];                     // rows >= M read row M - 1 again: their columns of D are never stored
#pragma unroll
    for (int t = 0; t < MT; ++t) xrow[t] = x + (long)min(t * 16 + r, M - 1) * ldx;
    f32x4_t acc[RG][MT];
#pragma unroll
    for (int c = 0; c < RG; ++c)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[c][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // loads are unmasked (clamped addresses only: K >= 32 keeps the first load, scale and x pieces of every row in
    // range).  Past the slice's end the codes are replaced by +0 where the load is consumed; the scale that meets them
    // is the row's first, a real one, and the x pieces are x's own first elements: the products are zero
    auto load_w = [&](S4W<RG, NU>& f, int k) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int ku = k + u * S4_UNIT, ko = ku + g * 64;
            if (ku < k1) {                      // wave-uniform: a unit wholly past the slice is not loaded, nor consumed
#pragma unroll
                for (int c = 0; c < RG; ++c) {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        f.v[c][2 * u + h] = __builtin_nontemporal_load(
                            reinterpret_cast<const u32x4_t*>(qrow[c] + ((ko + 32 * h + 32 <= k1 ? ko + 32 * h : 0) >> 1)));
                    if (pair)                   // K % 64 == 0: k1 % 64 == 0, both loads are inside the slice or neither
                        f.s[c][u] = *reinterpret_cast<const uint16_t*>(srow[c] + ((ko + 64 <= k1 ? ko : 0) >> 5));
                    else
                        f.s[c][u] = (unsigned)srow[c][(ko + 32 <= k1 ? ko : 0) >> 5] |
                                    (unsigned)srow[c][(ko + 64 <= k1 ? ko + 32 : 0) >> 5] << 8;
                }
            }
        }
    };
    auto load_x = [&](S4X<MT>& f, int ku, int h) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int ko = ku + g * 64 + h * 32 + p * 8;
            const int kc = ko + 8 <= k1 ? ko : 0;       // k1 % 32 == 0: the four pieces of a weight load end together
#pragma unroll
            for (int t = 0; t < MT; ++t) f.v[t][p] = *reinterpret_cast<const u16x8_t*>(xrow[t] + kc);
        }
    };
    auto mma = [&](const S4W<RG, NU>& w, int u, int h, const S4X<MT>& f, int ku) {
        const bool kv = ku + g * 64 + h * 32 + 32 <= k1;
        float s[RG];
#pragma unroll
        for (int c = 0; c < RG; ++c) s[c] = __uint_as_float(((w.s[c][u] >> (8 * h)) & 0xFFu) << 23);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int c = 0; c < RG; ++c) {
                const u16x8_t wq = cvt8(kv ? w.v[c][2 * u + h][p] : 0u, s[c]);
#pragma unroll
                for (int t = 0; t < MT; ++t)
                    acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wq),
                                                                       __builtin_bit_cast(bf16x8_t, f.v[t][p]), acc[c][t], 0, 0, 0);
            }
        }
    };

    if (k0 < k1) {                              // wave-uniform, as every branch on k below
        S4W<RG, NU> wa, wb;
        S4X<MT> xa, xb;                         // (xb is unused at MT = 4)
        // the units of one step: xa holds load 0 of unit ku on entry, load 1's x comes under its MFMAs, then the next unit's
        auto step = [&](const S4W<RG, NU>& w, int k) {
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int ku = k + u * S4_UNIT;
                if (ku < k1) {
                    if constexpr (MT == 4) {    // no ring: two entries of four row tiles do not fit beside two row groups
                        mma(w, u, 0, xa, ku);
                        load_x(xa, ku, 1);
                        mma(w, u, 1, xa, ku);
                        if (ku + S4_UNIT < k1) load_x(xa, ku + S4_UNIT, 0);
                    } else {
                        load_x(xb, ku, 1);
                        mma(w, u, 0, xa, ku);
                        if (ku + S4_UNIT < k1) load_x(xa, ku + S4_UNIT, 0);
                        mma(w, u, 1, xb, ku);
                    }
                }
            }
        };
        load_w(wa, k0);
        load_x(xa, k0, 0);
        int k = k0;
        while (true) {
            if (k + STEP >= k1) {
                step(wa, k);
                break;
            }
            load_w(wb, k + STEP);
            step(wa, k);
            k += STEP;
            if (k + STEP >= k1) {
                step(wb, k);
                break;
            }
            load_w(wa, k + STEP);
            step(wb, k);
            k += STEP;
        }
    }
#pragma unroll
    for (int c = 0; c < RG; ++c)
#pragma unroll
        for (int t = 0; t < MT; ++t) red[wv][c * MT + t][lane] = acc[c][t];
    __syncthreads();
    for (int i = wv; i < RG * MT; i += NW) {    // wave i % NW finishes tile i = (row group, row tile)
        f32x4_t v = red[0][i][lane];
#pragma unroll
        for (int j = 1; j < NW; ++j) v += red[j][i][lane];
        const int m = (i % MT) * 16 + r, n = n0 + (i / MT) * 16 + g * 4;
        if (m >= M || n >= N) continue;         // N % 8 == 0: n < N covers n .. n + 3
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = v[j];
        if (bias) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] += bias[n + j];     // scalar loads: a bias inside a flat arena is 4-byte aligned
        }
        if (act == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = gelu_tanh(bf2f(f2bf(o[j])));
        }
        if (res) {
            const u16x4_t rr = *reinterpret_cast<const u16x4_t*>(res + (long)m * ldc + n);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] += bf2f(rr[j]);
        }
        *reinterpret_cast<uint2*>(out + (long)m * ldc + n) = uint2{pk2bf(o[0], o[1]), pk2bf(o[2], o[3])};
    }
}

struct S4Args {
    const bf16_t* x; long ldx;
    const uint8_t* q; const uint8_t* sc;
    bf16_t* out; long ldc;
    int M, N, K, SL, pair;
    const float* bias; int act;
    const bf16_t* res;
};

template <int MT, int NW, int RG>
void skinny4_launch(const S4Args& a, hipStream_t st) {
    hipLaunchKernelGGL((gemm_skinny_fp4_kernel<MT, NW, RG>), dim3((unsigned)cdiv(a.N, 16 * RG)), dim3(NW * 64), 0, st, a.x,
                       a.ldx, a.q, a.sc, a.out, a.ldc, a.M, a.N, a.K, a.SL, a.pair, a.bias, a.act, a.res);
}

template <int MT, int RG>
void skinny4_launch_nw(int nw, const S4Args& a, hipStream_t st) {
    switch (nw) {
        case 2: skinny4_launch<MT, 2, RG>(a, st); break;
        case 3: skinny4_launch<MT, 3, RG>(a, st); break;
        case 4: skinny4_launch<MT, 4, RG>(a, st); break;
        case 6: skinny4_launch<MT, 6, RG>(a, st); break;
        default: skinny4_launch<MT, 8, RG>(a, st); break;
    }
}

template <int MT>
void skinny4_launch_rg(int rg, int nw, const S4Args& a, hipStream_t st) {
    if constexpr (MT < 4) {                     // (MT = 4 with two row groups spills at NW >= 6: not built)
        if (rg == 2) return skinny4_launch_nw<MT, 2>(nw, a, st);
    }
    skinny4_launch_nw<MT, 1>(nw, a, st);
}

}  // namespace

// w bf16 [N][K] contiguous -> q e2m1 codes [N][K / 2], sc e8m0 [N][K / 32] (the format of the header).  K % 32 == 0,
// N % 8 == 0, K >= 32, N >= 8; non-zero, and nothing launched, for every other shape.
PDNN_API int pdnn_quant_blocks_mxfp4(const bf16_t* w, int N, int K, uint8_t* q, uint8_t* sc, hipStream_t st) {
    if (!w || !q || !sc || K < 32 || K % 32 || N < 8 || N % 8) return (int)hipErrorInvalidValue;
    const long nblk = (long)N * (K / 32);
    hipLaunchKernelGGL(quant_blocks_mxfp4_kernel, dim3((unsigned)cdiv(nblk, 256)), dim3(256), 0, st, w, nblk, q, sc);
    PDNN_LAUNCH_RET;
}

// waves per block of pdnn_gemm_skinny_fp4 for (N, K) (0 on shapes it does not take); the slice of a wave is
// ceil(ceil(K / 256) / waves) * 256
PDNN_API int pdnn_gemm_skinny_fp4_plan(int N, int K) {
    if (K < 32 || N < 8 || K % 32 || N % 8) return 0;
    return skinny4_plan(N, K);
}

// x bf16 [M][K] (row stride ldx), q e2m1 [N][K / 2] and sc e8m0 [N][K / 32] contiguous, out bf16 [M][N] (row stride
// ldc), bias fp32 [N] or null, res bf16 with out's strides or null, act 0 / 2 (GELU).  groups: 16-row groups per wave, 1
// or (M <= 32) 2, 0 = the rule of (N, K, MT) (the result's bits do not depend on it; the measuring tools pass 1 and 2).  Non-zero,
// and nothing launched, for every other shape.
PDNN_API int pdnn_gemm_skinny_fp4_rg(const bf16_t* x, long ldx, const uint8_t* q, const uint8_t* sc, bf16_t* out,
                                         long ldc, int M, int N, int K, const float* bias, int act, const bf16_t* res,
                                         int groups, hipStream_t st) {
    if (!x || !q || !sc || !out || M < 1 || M > 64 || K < 32 || N < 8 || K % 32 || N % 8 || (act != 0 && act != 2) ||
        ldx < K || ldc < N || ldx % 8 || ldc % 4 || groups < 0 || groups > (M <= 32 ? 2 : 1))
        return (int)hipErrorInvalidValue;
    const int nw = skinny4_plan(N, K), mt = M <= 16 ? 1 : M <= 32 ? 2 : 4;
    const int rg = groups ? groups : skinny4_groups(N, K, mt);
    const int pair = K % 64 == 0 && (reinterpret_cast<uintptr_t>(sc) & 1) == 0;
    const S4Args a = {x, ldx, q, sc, out, ldc, M, N, K, (int)cdiv(cdiv(K, S4_UNIT), nw) * S4_UNIT, pair, bias, act, res};
    if (mt == 1)
        skinny4_launch_rg<1>(rg, nw, a, st);
    else if (mt == 2)
        skinny4_launch_rg<2>(rg, nw, a, st);
    else
        skinny4_launch_rg<4>(rg, nw, a, st);
    PDNN_LAUNCH_RET;
}

PDNN_API int pdnn_gemm_skinny_fp4(const bf16_t* x, long ldx, const uint8_t* q, const uint8_t* sc, bf16_t* out, long ldc,
                                  int M, int N, int K, const float* bias, int act, const bf16_t* res, hipStream_t st) {
    return pdnn_gemm_skinny_fp4_rg(x, ldx, q, sc, out, ldc, M, N, K, bias, act, res, 0, st);
}
