// Weight-only fp8 decode: the row quantiser and the skinny-M GEMM that streams its codes.
//     y[M][N] = act(x[M][K] . dq[N][K]^T + bias[N]) (+ res[M][N]),   1 <= M <= 64,
// x, res, y bf16, fp32 accumulation, and the weight stored as OCP e4m3fn codes q[N][K] (one byte per element) with one
// power-of-two scale per output row: dq[n][k] = value(q[n][k]) * inv[n].  gemm_skinny.hip reads every byte of the bf16
// shadow once and is bound by that stream; this kernel streams half the bytes.
//
// The format (pdnn_quant_rows_e4m3; ops/quant.py quantize_rows_reference is the same definition in torch).  For row n:
// amax = max_k |w[n][k]|; e = the smallest integer with amax 2^-e <= 448, i.e. with frexp(amax) = (m, x), m in [0.5, 1):
// e = x - 9 if m <= 0.875 else x - 8, clamped to [-100, 100], 0 for amax == 0; q = e4m3fn(w 2^-e) (round to nearest
// even; the product is exact and never above 448); inv = 2^e.  Every step but the one e4m3 rounding is exact, and dq is
// exactly a bf16 number: the GEMM below is an ordinary bf16 GEMM on dq.
// The quantiser runs one wave per row: 16-byte loads (a lane keeps up to 4 chunks of 16 elements, so rows up to 4096
// elements are read once; longer rows re-read their tail), the amax of the bf16 magnitudes as integers by a wave
// reduction, the exponent rule on the bf16 exponent and mantissa fields, v_cvt_pk_fp8_f32 and 16-byte stores.
//
// MFMA orientation, as gemm_skinny.hip: v_mfma_f32_16x16x32_bf16 with the 16 weight rows as the A operand and 16 rows
// of x as the B operand, D[n][m]: lane l holds D[n = 4 (l >> 4) + j][m = l & 15], four consecutive columns of one
// output row.  MT in {1, 2, 4} (compile time) row tiles of x; rows >= M read row M - 1 again (clamped addresses): a
// column of D depends on its own row of x only, and those columns are never stored.
//
// Stream and reduction permutation.  The reduction unit is 128 elements: lane (r = l & 15, g = l >> 4) owns weight
// row n0 + r and bytes [32 g, 32 g + 32) of the row's 128-byte line, two back-to-back nontemporal 16-byte loads
// straight to VGPRs (no LDS stage: the operand is not shared between waves); the four lanes of a row cover one whole
// cache line per unit.  MFMA h (0..3) of a unit takes the lane's elements [32 g + 8 h, 32 g + 8 h + 8); the x fragment
// is read from x's row at the same element offsets (bf16: four 16-byte loads per lane, unit and row tile), so both
// operands of an MFMA see the same 32 reduction indices.
//
// Conversion in registers: v_cvt_scalef32_pk_bf16_fp8, two codes per instruction, with inv[n0 + r] as its scale operand
// (lane r owns weight row n0 + r; the scale is a power of two, so the result is exactly dq and no multiply is left
// for the epilogue).  The other candidate, v_cvt_pk_f32_fp8 + v_cvt_pk_bf16_f32 with the fp32 sum multiplied by inv in
// the epilogue, takes twice the conversion instructions; both pass the fp64 test, and this one measured faster on the
// LM head and the same within 2% on the block linears.  Those figures are of an earlier revision of this kernel, not
// its current times: 13.8 against 15.0 us at N = 50304, K = 768, M = 1 and 16.3 against 17.4 at M = 8, where section 1
// of profiles/gemm_skinny_fp8.txt now has 12.7 and 14.4 (section 4 there: recorded once, the other conversion is not
// in the tree).
//
// Bytes in flight.  A wave keeps two steps of weights in registers, the one the MFMAs read and the next one in flight.
// A step is four units (8 loads per lane: 8 KiB per wave and 16 rows) at MT <= 2 and two units at MT = 4, where the x
// fragments take the registers.  x (<= 64 rows, from L2) runs one unit ahead of the MFMAs in a two-unit ring.
// Resource usage (the compiler's kernel-resource-usage report, gfx950; VGPRs + AGPRs at NW <= 4, VGPRs at NW = 6, 8; no
// spills, no scratch; two waves per SIMD everywhere, which the register rings cost):
//     MT = 1 (4 units / step):  171 + 12, 176     2 waves / SIMD      LDS NW x 1 KiB
//     MT = 2 (4 units / step):  224 + 24, 237     2 waves / SIMD      LDS NW x 2 KiB
//     MT = 4 (2 units / step):  204 + 48, 228     2 waves / SIMD      LDS NW x 4 KiB
// MT = 4 (M > 32) keeps one x unit, not a ring, and 4 KiB of weights per step: with four units per step it compiles to
// 256 VGPRs with spills at NW >= 6 and one wave per SIMD below, so it stays under the 8 KiB of the other two.
// A unit wholly past a wave's slice is neither loaded nor consumed (a one-unit slice issues two weight loads, not eight).
//
// Partition of K, a function of (N, K) only (pdnn_gemm_skinny_fp8_plan).  A block has NW in {2, 3, 4, 6, 8} waves;
// wave v reduces the slice [v SL, min((v + 1) SL, K)), SL = ceil(units / NW) * 128, MFMA after MFMA in ascending
// order into one fp32 accumulator per row tile; an empty slice contributes zeros.  NW is the smallest count that gives
// the grid >= 1024 waves and divides the units of K, else the smallest with >= 1024 waves and NW <= units, else the
// largest NW <= units, else 2.  The NW partial tiles go through LDS and are added in wave order by wave t % NW for
// row tile t, which applies the epilogue of gemm_skinny.hip: v = acc; v += bias; GELU (gelu_tanh) of the
// bf16-rounded v; v += res; round to nearest even.  No atomics, nothing depends on M or MT: row b of an M-row call has
// the bits of the 1-row call on that row.
//
// Edges: the last group when N % 16 == 8 (weight rows and inv clamped to N - 1, their columns never stored), the K tail
// (K % 16 == 0: a 16-byte weight load, and the two x loads that match it, past the slice's end are issued at offset 0
// of the row; the codes are replaced by +0, which the x values there multiply to zero) and rows >= M.  So a tail's
// zeros meet x[m][0 .. 15]: a non-finite activation there makes row m's whole output non-finite, as in gemm_skinny.hip
// (a row with a non-finite activation is outside both kernels' contract).  No access leaves q[N][K], inv[N], x[M][K]
// (+ ldx), [M][N] (+ ldc).
#include "gemm_common.h"

namespace {
using pg::gelu_tanh;

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

constexpr int S8_UNIT = 128;        // reduction elements of one load pair = four MFMAs
constexpr int S8_MIN_WAVES = 1024;  // waves the grid should reach (4 per CU)
constexpr int QR_KEEP = 4;          // 16-element chunks of a row a quantiser lane keeps in registers

// ------------------------------------------------------------------------------------------------ quantiser
__device__ __forceinline__ unsigned amax16(const u16x8_t& a, const u16x8_t& b, unsigned m) {
#pragma unroll
    for (int j = 0; j < 8; ++j) m = max(m, max((unsigned)(a[j] & 0x7FFF), (unsigned)(b[j] & 0x7FFF)));
    return m;
}

__device__ __forceinline__ u32x4_t codes16(const u16x8_t& a, const u16x8_t& b, float s) {
    u32x4_t o;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(a[4 * d]) * s, bf2f(a[4 * d + 1]) * s, lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(a[4 * d + 2]) * s, bf2f(a[4 * d + 3]) * s, lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(b[4 * d]) * s, bf2f(b[4 * d + 1]) * s, hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(b[4 * d + 2]) * s, bf2f(b[4 * d + 3]) * s, hi, true);
        o[d] = (unsigned)lo;
        o[2 + d] = (unsigned)hi;
    }
    return o;
}

__global__ void __launch_bounds__(256) quant_rows_e4m3_kernel(const bf16_t* __restrict__ w, int N, int K,
                                                              uint8_t* __restrict__ q, float* __restrict__ inv) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;                       // wave-uniform
    const bf16_t* wr = w + (long)row * K;
    uint8_t* qr = q + (long)row * K;
    const int nch = K / 16;
    auto ld = [&](int c, int h) { return *reinterpret_cast<const u16x8_t*>(wr + 16 * c + 8 * h); };
    u16x8_t keep[QR_KEEP][2];
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < QR_KEEP; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            keep[i][0] = ld(c, 0);
            keep[i][1] = ld(c, 1);
            m = amax16(keep[i][0], keep[i][1], m);
        }
    }
    for (int c = lane + 64 * QR_KEEP; c < nch; c += 64) m = amax16(ld(c, 0), ld(c, 1), m);
    // the magnitudes order as their bit patterns (< 2^15: exact in fp32)
    const unsigned a = (unsigned)wave_max((float)m);
    int e = 0;
    if (a) {        // frexp: m = (1 + mant / 128) / 2, x = E - 126; m <= 0.875 <=> mant <= 96; a subnormal clamps to -100
        e = (int)(a >> 7) - 126 - ((a & 127) <= 96 ? 9 : 8);
        e = min(max(e, -100), 100);
    }
    const float s = __uint_as_float((unsigned)(127 - e) << 23);
    if (lane == 0) inv[row] = __uint_as_float((unsigned)(127 + e) << 23);
#pragma unroll
    for (int i = 0; i < QR_KEEP; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) *reinterpret_cast<u32x4_t*>(qr + 16 * c) = codes16(keep[i][0], keep[i][1], s);
    }
    for (int c = lane + 64 * QR_KEEP; c < nch; c += 64) *reinterpret_cast<u32x4_t*>(qr + 16 * c) = codes16(ld(c, 0), ld(c, 1), s);
}

// ------------------------------------------------------------------------------------------------ GEMM
// waves per block for (N, K); the slice of a wave is then ceil(units / NW) * 128
int skinny8_plan(int N, int K) {
    const long groups = cdiv(N, 16), units = cdiv(K, S8_UNIT);
    const int cands[5] = {2, 3, 4, 6, 8};
    for (int c : cands)
        if (groups * c >= S8_MIN_WAVES && units % c == 0) return c;
    for (int c : cands)
        if (groups * c >= S8_MIN_WAVES && c <= units) return c;
    for (int i = 4; i >= 0; --i)
        if (cands[i] <= units) return cands[i];
    return 2;
}

// 8 e4m3 codes (two dwords) of a weight row -> 8 bf16 of dq, exact: sc = the row's inv, a power of two
typedef __bf16 s8_bf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x8_t cvt8(unsigned a, unsigned b, float sc) {
    const s8_bf2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, sc, false), p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, sc, true);
    const s8_bf2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, sc, false), p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, sc, true);
    const u32x4_t o = {__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1), __builtin_bit_cast(unsigned, p2),
                       __builtin_bit_cast(unsigned, p3)};
    return __builtin_bit_cast(u16x8_t, o);
}

template <int NU>
struct S8W {
    u32x4_t v[2 * NU];          // load i: unit i >> 1, elements [32 g + 16 (i & 1), + 16) of it
};
template <int MT>
struct S8X {
    u16x8_t v[MT][4];           // one unit: piece p = elements [32 g + 8 p, + 8), the B operand of the unit's MFMA p
};

template <int MT, int NW>
__global__ void __launch_bounds__(NW * 64) gemm_skinny_fp8_kernel(const bf16_t* __restrict__ x, long ldx,
                                                                  const uint8_t* __restrict__ q,
                                                                  const float* __restrict__ inv, bf16_t* __restrict__ out,
                                                                  long ldc, int M, int N, int K, int SL,
                                                                  const float* __restrict__ bias, int act,
                                                                  const bf16_t* __restrict__ res) {
    constexpr int NU = MT == 4 ? 2 : 4;         // units per step (even: the x ring below starts every step on xa)
    constexpr int STEP = NU * S8_UNIT;
    __shared__ __attribute__((aligned(16))) f32x4_t red[NW][MT][64];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int k0 = min(wv * SL, K), k1 = min(k0 + SL, K);
    const uint8_t* qrow = q + (long)min(n0 + r, N - 1) * K;
    const float sc = inv[min(n0 + r, N - 1)];   // lane r owns weight row n0 + r: its scale rides in the conversion
    const bf16_t* xrow[MT];                     // rows >= M read row M - 1 again: their columns of D are never stored
#pragma unroll
    for (int t = 0; t < MT; ++t) xrow[t] = x + (long)min(t * 16 + r, M - 1) * ldx;
    f32x4_t acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // loads are unmasked (clamped addresses only: K >= 16 keeps offset 0 in range for every row).  Past the slice's end
    // the codes are replaced by +0 where the unit is consumed, so that nothing waits for a load between its issue and
    // the MFMAs before it; the x pieces that meet them are x's own first elements, and their products are zero
    auto load_w = [&](S8W<NU>& f, int k) {
#pragma unroll
        for (int i = 0; i < 2 * NU; ++i) {
            const int ko = k + (i >> 1) * S8_UNIT + g * 32 + (i & 1) * 16;
            if (k + (i >> 1) * S8_UNIT < k1)    // wave-uniform: a unit wholly past the slice is not loaded, nor consumed
                f.v[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(qrow + (ko + 16 <= k1 ? ko : 0)));
        }
    };
    auto load_x = [&](S8X<MT>& f, int ku) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int ko = ku + g * 32 + p * 8;
            const int kc = ko + 8 <= k1 ? ko : 0;       // k1 % 16 == 0: both pieces of a weight load end together
#pragma unroll
            for (int t = 0; t < MT; ++t) f.v[t][p] = *reinterpret_cast<const u16x8_t*>(xrow[t] + kc);
        }
    };
    auto mma = [&](const u32x4_t& w0, const u32x4_t& w1, const S8X<MT>& f, int ku) {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const bool kv = ku + g * 32 + (h >> 1) * 16 + 16 <= k1;
            const u32x4_t& wl = h < 2 ? w0 : w1;
            const u16x8_t wq = cvt8(kv ? wl[2 * (h & 1)] : 0u, kv ? wl[2 * (h & 1) + 1] : 0u, sc);
#pragma unroll
            for (int t = 0; t < MT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wq),
                                                                 __builtin_bit_cast(bf16x8_t, f.v[t][h]), acc[t], 0, 0, 0);
        }
    };

    if (k0 < k1) {                              // wave-uniform, as every branch on k below
        S8W<NU> wa, wb;
        S8X<MT> xa, xb;                         // (xb is unused at MT = 4)
        // the units of one step, in pairs: xa holds unit ku on entry, xb is loaded under its MFMAs, then xa again
        auto step = [&](const S8W<NU>& w, int k) {
#pragma unroll
            for (int u = 0; u < NU; u += 2) {
                const int ku = k + u * S8_UNIT;
                if constexpr (MT == 4) {        // no ring: two units of four row tiles do not fit the registers
                    if (ku < k1) mma(w.v[2 * u], w.v[2 * u + 1], xa, ku);
                    if (ku + S8_UNIT < k1) {
                        load_x(xa, ku + S8_UNIT);
                        mma(w.v[2 * u + 2], w.v[2 * u + 3], xa, ku + S8_UNIT);
                    }
                    if (ku + 2 * S8_UNIT < k1) load_x(xa, ku + 2 * S8_UNIT);
                } else if (ku < k1) {
                    const bool two = ku + S8_UNIT < k1;
                    if (two) load_x(xb, ku + S8_UNIT);
                    mma(w.v[2 * u], w.v[2 * u + 1], xa, ku);
                    if (two) {
                        if (ku + 2 * S8_UNIT < k1) load_x(xa, ku + 2 * S8_UNIT);
                        mma(w.v[2 * u + 2], w.v[2 * u + 3], xb, ku + S8_UNIT);
                    }
                }
            }
        };
        load_w(wa, k0);
        load_x(xa, k0);
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
    for (int t = 0; t < MT; ++t) red[wv][t][lane] = acc[t];
    __syncthreads();
    for (int t = wv; t < MT; t += NW) {         // wave t % NW finishes row tile t
        f32x4_t v = red[0][t][lane];
#pragma unroll
        for (int i = 1; i < NW; ++i) v += red[i][t][lane];
        const int m = t * 16 + r, n = n0 + g * 4;
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

struct S8Args {
    const bf16_t* x; long ldx;
    const uint8_t* q; const float* inv;
    bf16_t* out; long ldc;
    int M, N, K, SL;
    const float* bias; int act;
    const bf16_t* res;
};

template <int MT, int NW>
void skinny8_launch(const S8Args& a, hipStream_t st) {
    hipLaunchKernelGGL((gemm_skinny_fp8_kernel<MT, NW>), dim3((unsigned)cdiv(a.N, 16)), dim3(NW * 64), 0, st, a.x, a.ldx,
                       a.q, a.inv, a.out, a.ldc, a.M, a.N, a.K, a.SL, a.bias, a.act, a.res);
}

template <int MT>
void skinny8_launch_nw(int nw, const S8Args& a, hipStream_t st) {
    switch (nw) {
        case 2: skinny8_launch<MT, 2>(a, st); break;
        case 3: skinny8_launch<MT, 3>(a, st); break;
        case 4: skinny8_launch<MT, 4>(a, st); break;
        case 6: skinny8_launch<MT, 6>(a, st); break;
        default: skinny8_launch<MT, 8>(a, st); break;
    }
}

}  // namespace

// w bf16 [N][K] contiguous -> q e4m3fn codes [N][K], inv fp32 [N] (the format of the header).  K % 16 == 0, N % 8 == 0,
// K >= 16, N >= 8; non-zero, and nothing launched, for every other shape.
PDNN_API int pdnn_quant_rows_e4m3(const bf16_t* w, int N, int K, uint8_t* q, float* inv, hipStream_t st) {
    if (!w || !q || !inv || K < 16 || K % 16 || N < 8 || N % 8) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(quant_rows_e4m3_kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, st, w, N, K, q, inv);
    PDNN_LAUNCH_RET;
}

// waves per block of pdnn_gemm_skinny_fp8 for (N, K) (0 on shapes it does not take); the slice of a wave is
// ceil(ceil(K / 128) / waves) * 128
PDNN_API int pdnn_gemm_skinny_fp8_plan(int N, int K) {
    if (K < 16 || N < 8 || K % 16 || N % 8) return 0;
    return skinny8_plan(N, K);
}

// x bf16 [M][K] (row stride ldx), q e4m3fn [N][K] contiguous, inv fp32 [N], out bf16 [M][N] (row stride ldc), bias fp32
// [N] or null, res bf16 with out's strides or null, act 0 / 2 (GELU).  Non-zero, and nothing launched, for every other
// shape.
PDNN_API int pdnn_gemm_skinny_fp8(const bf16_t* x, long ldx, const uint8_t* q, const float* inv, bf16_t* out, long ldc,
                                  int M, int N, int K, const float* bias, int act, const bf16_t* res, hipStream_t st) {
    if (!x || !q || !inv || !out || M < 1 || M > 64 || K < 16 || N < 8 || K % 16 || N % 8 || (act != 0 && act != 2) ||
        ldx < K || ldc < N || ldx % 8 || ldc % 4)
        return (int)hipErrorInvalidValue;
    const int nw = skinny8_plan(N, K);
    const S8Args a = {x, ldx, q, inv, out, ldc, M, N, K, (int)cdiv(cdiv(K, S8_UNIT), nw) * S8_UNIT, bias, act, res};
    if (M <= 16)
        skinny8_launch_nw<1>(nw, a, st);
    else if (M <= 32)
        skinny8_launch_nw<2>(nw, a, st);
    else
        skinny8_launch_nw<4>(nw, a, st);
    PDNN_LAUNCH_RET;
}
