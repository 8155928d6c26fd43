// Skinny-M weight-streaming GEMM for the M = B linears of GPT-2 decode:
//     y[M][N] = act(x[M][K] . w[N][K]^T + bias[N]) (+ res[M][N]),   1 <= M <= 64,
// bf16 operands, fp32 accumulation, bf16 output.  w is the row-major [N][K] shadow the other engines read (no second
// copy, no re-layout); x and out are row-strided (ldx, ldc).  The 128-row MFMA tile of the other engines launches 6-24
// blocks for these shapes and streams the weights at a small fraction of the HBM rate; here every weight byte is read
// once, by a grid of one block per 16 weight rows, and the work of a block is only the stream.
//
// MFMA orientation.  v_mfma_f32_16x16x32_bf16 with the 16 weight rows as the A operand and 16 rows of x as the B
// operand: D[n][m], lane l holds D[n = 4 (l >> 4) + j][m = l & 15], j = 0..3, so a lane ends with four consecutive
// columns of one output row: one 8-byte store and one 8-byte residual load.  MT in {1, 2, 4}
// (compile time) is the number of 16-row tiles of x; rows >= M are zeros in the fragment (their addresses are clamped
// to row M - 1 and the value is replaced by zero), and never stored.
//
// Reduction permutation.  A lane (r = l & 15, g = l >> 4) owns row r and, in every 64-element unit of K, the 16
// elements [16 g, 16 g + 16): two back-to-back 16-byte loads of 32 contiguous bytes.  The four lanes of a row then
// cover 128 contiguous bytes (one cache line) in each load instruction of the pair, every 32-byte sector of the line
// in the first of the two, instead of the 64-byte half lines of the natural fragment order.  MFMA h (0, 1) of a unit
// takes the lane's elements [16 g + 8 h, 16 g + 8 h + 8): its 32 reduction indices are {16 g + 8 h + j}, the same
// for the x fragment, which is loaded with the same addresses from x's row.
//
// Partition of K (a function of (N, K) only: skinny_plan below, mirrored by tests/gemm_skinny_ref.py).  A block has NW
// in {4, 6, 8, 12} waves (12: the most that leaves a wave 170 VGPRs); wave v reduces the slice [v SL, min((v + 1) SL, K)),
// SL a multiple of 64, MFMA after MFMA in ascending unit order into one fp32 accumulator per row tile; a wave whose slice is empty contributes zeros.  The
// NW partial tiles go through LDS and are added in wave order 0, 1, .. by the threads of the first MT waves, which
// then apply the epilogue of the other engines: v = acc; v += bias; GELU (gelu_tanh of gemm_common.h) of the
// bf16-rounded v; v += res; round to nearest even.  No atomics, no cross-block reduction, nothing depends on M or MT:
// the bits of output row b are those of the 1-row call on that row, whatever the other rows hold.
// NW is the smallest count that gives the chip >= 1024 waves (4 per CU) and divides the 64-element units of K, so
// that N = 768, K = 3072 (48 column groups) runs 576 waves of 8 KiB each and needs no split of K across blocks.
//
// Streaming.  Weights go straight to VGPRs (nontemporal 16-byte loads: each byte is used once), no LDS stage: the
// operand is not shared between waves.  A wave keeps two steps in registers, the one the MFMAs read and the next one
// in flight; a step is two units (8 KiB of weights per wave and 16 rows; one unit at MT = 4, where the x fragments
// take the registers).  x (<= 64 rows) comes from L2.
//
// Edges: the last column group when N % 16 == 8 (weight rows clamped to N - 1, their columns never stored), the K tail
// of a slice (a 16-byte load that would pass the slice's end is issued at offset 0 of the row and replaced by zero)
// and rows >= M.  No access leaves [N][K], [M][K] (+ ldx), [M][N] (+ ldc).
#include "gemm_common.h"

namespace {
using pg::gelu_tanh;

constexpr int SK_UNIT = 64;         // reduction elements of one load pair = two MFMAs
constexpr int SK_MIN_WAVES = 1024;  // waves the grid should reach (4 per CU)

// waves per block for (N, K); the slice of a wave is then ceil(units / NW) * 64
int skinny_plan(int N, int K) {
    const long groups = cdiv(N, 16), units = cdiv(K, SK_UNIT);
    const int cands[4] = {4, 6, 8, 12};
    for (int c : cands)
        if (groups * c >= SK_MIN_WAVES && units % c == 0) return c;
    for (int c : cands)
        if (groups * c >= SK_MIN_WAVES && c <= units) return c;
    for (int i = 3; i >= 0; --i)
        if (cands[i] <= units) return cands[i];
    return 4;
}

template <int MT, int NL>
struct SkFrag {
    u16x8_t w[NL];
    u16x8_t x[MT][NL];
};

template <int MT, int NW>
__global__ void __launch_bounds__(NW * 64) gemm_skinny_kernel(const bf16_t* __restrict__ x, long ldx,
                                                              const bf16_t* __restrict__ w, bf16_t* __restrict__ out,
                                                              long ldc, int M, int N, int K, int SL,
                                                              const float* __restrict__ bias, int act,
                                                              const bf16_t* __restrict__ res) {
    constexpr int NU = MT == 4 ? 1 : 2;         // units per step
    constexpr int NL = 2 * NU;                  // 16-byte loads per row and step
    constexpr int STEP = NU * SK_UNIT;
    __shared__ __attribute__((aligned(16))) f32x4_t red[NW][MT][64];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int k0 = min(wv * SL, K), k1 = min(k0 + SL, K);
    const bf16_t* wrow = w + (long)min(n0 + r, N - 1) * K;
    const bf16_t* xrow[MT];
    bool mv[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        mv[t] = t * 16 + r < M;
        xrow[t] = x + (long)min(t * 16 + r, M - 1) * ldx;
    }
    const u16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
    f32x4_t acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // the loads of a step, unmasked (clamped addresses only): the masks are applied where the step is consumed, so
    // that nothing waits for a load between its issue and the MFMAs of the step before
    auto koff = [&](int k, int q) { return k + (q >> 1) * SK_UNIT + g * 16 + (q & 1) * 8; };
    auto load = [&](SkFrag<MT, NL>& f, int k) {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int ko = koff(k, q);
            const int kc = ko + 8 <= k1 ? ko : 0;       // in range for every row: K >= 8
            f.w[q] = __builtin_nontemporal_load(reinterpret_cast<const u16x8_t*>(wrow + kc));
#pragma unroll
            for (int t = 0; t < MT; ++t) f.x[t][q] = *reinterpret_cast<const u16x8_t*>(xrow[t] + kc);
        }
    };
    auto mma = [&](const SkFrag<MT, NL>& f, int k) {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const bool kv = koff(k, q) + 8 <= k1;
            const u16x8_t wq = kv ? f.w[q] : zero;
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const u16x8_t xq = (kv && mv[t]) ? f.x[t][q] : zero;
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wq),
                                                                 __builtin_bit_cast(bf16x8_t, xq), acc[t], 0, 0, 0);
            }
        }
    };

    if (k0 < k1) {                              // wave-uniform
        SkFrag<MT, NL> fa, fb;
        load(fa, k0);
        int k = k0;
        while (true) {
            if (k + STEP >= k1) {
                mma(fa, k);
                break;
            }
            load(fb, k + STEP);
            mma(fa, k);
            k += STEP;
            if (k + STEP >= k1) {
                mma(fb, k);
                break;
            }
            load(fa, k + STEP);
            mma(fb, k);
            k += STEP;
        }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) red[wv][t][lane] = acc[t];
    __syncthreads();
    if (tid >= MT * 64) return;                 // NW >= 4 >= MT: wave t finishes row tile t
    f32x4_t v = red[0][wv][lane];
#pragma unroll
    for (int i = 1; i < NW; ++i) v += red[i][wv][lane];
    const int m = wv * 16 + r, n = n0 + g * 4;
    if (m >= M || n >= N) return;               // N % 8 == 0: n < N covers n .. n + 3
    float o[4] = {v[0], v[1], v[2], v[3]};
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

template <int MT, int NW>
void skinny_launch(const bf16_t* x, long ldx, const bf16_t* w, bf16_t* out, long ldc, int M, int N, int K, int SL,
                   const float* bias, int act, const bf16_t* res, hipStream_t st) {
    hipLaunchKernelGGL((gemm_skinny_kernel<MT, NW>), dim3((unsigned)cdiv(N, 16)), dim3(NW * 64), 0, st, x, ldx, w, out,
                       ldc, M, N, K, SL, bias, act, res);
}

template <int MT>
void skinny_launch_nw(int nw, const bf16_t* x, long ldx, const bf16_t* w, bf16_t* out, long ldc, int M, int N, int K,
                      int SL, const float* bias, int act, const bf16_t* res, hipStream_t st) {
    switch (nw) {
        case 4: skinny_launch<MT, 4>(x, ldx, w, out, ldc, M, N, K, SL, bias, act, res, st); break;
        case 6: skinny_launch<MT, 6>(x, ldx, w, out, ldc, M, N, K, SL, bias, act, res, st); break;
        case 8: skinny_launch<MT, 8>(x, ldx, w, out, ldc, M, N, K, SL, bias, act, res, st); break;
        default: skinny_launch<MT, 12>(x, ldx, w, out, ldc, M, N, K, SL, bias, act, res, st); break;
    }
}

}  // namespace

// waves per block of pdnn_gemm_skinny for (N, K) (0 on shapes it does not take); the slice of a wave is
// ceil(ceil(K / 64) / waves) * 64
PDNN_API int pdnn_gemm_skinny_plan(int N, int K) {
    if (K < 8 || N < 8 || K % 8 || N % 8) return 0;
    return skinny_plan(N, K);
}

// x bf16 [M][K] (row stride ldx), w bf16 [N][K] contiguous, out bf16 [M][N] (row stride ldc), bias fp32 [N] or null,
// res bf16 with out's strides or null, act 0 / 2 (GELU).  Non-zero, and nothing launched, for every other shape.
PDNN_API int pdnn_gemm_skinny(const bf16_t* x, long ldx, const bf16_t* w, bf16_t* out, long ldc, int M, int N, int K,
                              const float* bias, int act, const bf16_t* res, hipStream_t st) {
    if (!x || !w || !out || M < 1 || M > 64 || K < 8 || N < 8 || K % 8 || N % 8 || (act != 0 && act != 2) ||
        ldx < K || ldc < N || ldx % 8 || ldc % 4)
        return (int)hipErrorInvalidValue;
    const int nw = skinny_plan(N, K);
    const int SL = (int)cdiv(cdiv(K, SK_UNIT), nw) * SK_UNIT;
    if (M <= 16)
        skinny_launch_nw<1>(nw, x, ldx, w, out, ldc, M, N, K, SL, bias, act, res, st);
    else if (M <= 32)
        skinny_launch_nw<2>(nw, x, ldx, w, out, ldc, M, N, K, SL, bias, act, res, st);
    else
        skinny_launch_nw<4>(nw, x, ldx, w, out, ldc, M, N, K, SL, bias, act, res, st);
    PDNN_LAUNCH_RET;
}
