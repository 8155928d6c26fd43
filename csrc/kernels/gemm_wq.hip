// Quantised-weight prefill: the weight-only GEMM for many rows, on the stored forms of ops/quant.py unchanged.
//     y[M][N] = act(x[M][K] . dq[N][K]^T + bias[N]) (+ res[M][N]),   any M >= 1,
// x, res, y bf16, fp32 accumulation, bias fp32, act 0 / 2 (GELU of the bf16-rounded pre-activation, no aux), and the
// weight either e4m3fn codes q[N][K] with one power-of-two scale per row inv[N] (gemm_skinny_fp8.hip's format, K % 16
// == 0) or MXFP4, e2m1 codes q[N][K / 2] with one e8m0 scale per 32 reduction elements sc[N][K / 32]
// (gemm_skinny_fp4.hip's format, K % 32 == 0).  dq is exactly a bf16 number in both: this is an ordinary bf16 GEMM on
// dq, the wide-M sibling of the two skinny kernels (which stop at 64 rows and stream the weight once per call).
//
// Tile.  Output-stationary, BT x BT with BT = 128 (or 64, below), 256 threads = four waves as 2 x 2, each wave BT / 2 x
// BT / 2 on v_mfma_f32_16x16x32_bf16 with 16 weight rows as the A operand and 16 rows of x as the B operand, D[n][m]:
// lane l holds D[n = 4 (l >> 4) + j][m = l & 15], four neighbouring columns of one output row, one 8-byte store.
// At BT = 128 a wave has 4 x 4 accumulator fragments (64 registers) and reads 8 fragments from LDS for 16 MFMAs; at
// BT = 64, 2 x 2 fragments and 4 reads for 4 MFMAs.
// The 64 x 64 instantiation runs where the 128 x 128 grid would not fill the 256 CUs one and a half times:
// ceil(M / 128) ceil(N / 128) < 384 (wq_tile, exported as pdnn_gemm_wq_plan; e.g. M = 128 on GPT-2's proj: 6 blocks
// of 128 x 128, 24 of 64 x 64).  It converts every weight element ceil(M / 64) times, not ceil(M / 128), and reads twice
// the LDS bytes per MFMA: it is the latency tile, not the throughput tile.  The threshold is measured
// (profiles/gemm_wq.txt, section 1, the t64 / t128 columns): with both tiles forced, 64 x 64 won on every GPT-2 small and
// medium linear up to 256 blocks of 128 x 128 (fc of medium at M = 1024: 22.4 against 28.3 us), tied at 384 (proj of
// small at M = 8192) and lost from 512 (proj of medium at M = 8192: 39.4 against 32.6 us).
//
// No split over K, no atomics.  The k-step is 64 elements (one row of the k-major LDS image of gemm_common.h:
// kimg_off / frag_kmajor, 128-byte rows with the chunk swizzle); a block walks ceil(K / 64) steps in order and every
// output element is one fp32 accumulator that takes the two MFMAs of every step in order, in both instantiations, the
// zero-filled tail included.  So the result is bitwise repeatable, and a row's bits depend neither on M, nor on the
// other rows, nor on the tile: chunked ingest of a prompt is independent of the chunking as far as the linears go.
//
// Weights move as codes and are converted once per block.  One load is 16 bytes of one weight row, straight to VGPRs:
// 16 e4m3 elements (four loads per row and k-step) or 32 e2m1 elements (two), the latter exactly one scale block, whose
// scale byte is loaded with it; the fp8 row scale is loaded once per block (a lane's rows do not change with k).  Load
// i = tid + 256 j of a step is row i / LPR, part i % LPR: 2 | 1 | 1 | 0.5 loads per lane for (128, fp8) | (128, fp4) |
// (64, fp8) | (64, fp4; waves 0 and 1 only).  They are ordinary loads, not nontemporal: every row tile reads the same
// weight tile, which should stay in L2.  The lane converts with v_cvt_scalef32_pk_bf16_fp8 / _fp4, the scale riding in
// the conversion (a power of two: what reaches LDS is exactly dq), and writes 2 | 4 16-byte chunks of bf16 into the
// k-major image.  x goes the same way without the conversion: 16-byte loads to registers (BT / 32 per lane and step),
// then into its own k-major image.  Both images are double-buffered (2 x 2 x BT x 128 bytes: 64 KiB at BT = 128, 32 KiB
// at 64); the loads of step i + 1 are issued before the MFMAs of step i, the conversions and the weight image's
// writes sit between the two MFMA halves of step i, x's writes after them, and one barrier ends the step.
//
// Edges.  Weight rows >= N and x rows >= M are clamped to the last row (their columns / rows of D are never stored);
// a load whose first element is at or past K is not issued: the weight registers hold the code 0 (+0 under any
// scale), x's hold +0, so the tail of the last step adds +0 products.  K % 16 (32) == 0 makes every load whole.  Stores
// are masked by m < M and n < N (N % 8 == 0: n < N covers n .. n + 3).  No access leaves q, inv / sc, x[M][K] (+ ldx),
// bias[N], [M][N] (+ ldc).
//
// Epilogue, one function for both formats, the order of gemm_common.h / tests/gemm_ref.py: v = acc; v += bias; GELU
// (gelu_tanh) of the bf16-rounded v; v += res; round to nearest even.
//
// Resource usage (the compiler's kernel-resource-usage report, gfx950, built without packed fp32 ops as the siblings;
// no spills and no scratch in any instantiation; __launch_bounds__(256, 2)):
//     128 x 128 fp8:  148 VGPRs, 0 AGPRs, 64 KiB LDS    2 waves / SIMD = 2 blocks / CU (128 of the CU's 160 KiB)
//     128 x 128 fp4:  142 VGPRs, 0 AGPRs, 64 KiB LDS    2
//      64 x  64 fp8:   66 VGPRs, 0 AGPRs, 32 KiB LDS    5 by registers, 5 blocks / CU by LDS
//      64 x  64 fp4:   76 VGPRs, 0 AGPRs, 32 KiB LDS    5
#include "gemm_common.h"

namespace {
using pg::BK;
using pg::frag_kmajor;
using pg::gelu_tanh;
using pg::kimg_off;

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __bf16 wq_bf2 __attribute__((ext_vector_type(2)));

constexpr int WQ_NT = 256;          // threads of a block: four waves as 2 (rows of x) x 2 (weight rows)
constexpr int WQ_MIN_BLOCKS = 384;  // 128 x 128 blocks below which the 64 x 64 tile runs (1.5 per CU; measured, above)

// the tile of (M, N): a rule of the shape alone
int wq_tile(long M, long N) { return cdiv(M, 128) * cdiv(N, 128) >= WQ_MIN_BLOCKS ? 128 : 64; }

__device__ __forceinline__ u16x8_t wq_pack(wq_bf2 p0, wq_bf2 p1, wq_bf2 p2, wq_bf2 p3) {
    const u32x4_t o = {__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1), __builtin_bit_cast(unsigned, p2),
                       __builtin_bit_cast(unsigned, p3)};
    return __builtin_bit_cast(u16x8_t, o);
}

// The load and convert stage, the only part in which the two formats differ.  LPR loads of 16 bytes per weight row and
// k-step, CPL 8-element chunks of bf16 out of each.
template <bool FP4>
struct WqFmt;
template <>
struct WqFmt<false> {       // e4m3fn codes, scl = inv fp32 [N]
    static constexpr int LPR = 4, CPL = 2;
    const uint8_t* p;       // the lane's 16 bytes of step 0
    float s;                // the row's scale, for every step
    u32x4_t v;
    __device__ __forceinline__ void init(const uint8_t* q, const void* scl, long row, int part, int K) {
        p = q + row * K + part * 16;
        s = static_cast<const float*>(scl)[row];
    }
    __device__ __forceinline__ void load(int k0, bool in) {
        v = in ? *reinterpret_cast<const u32x4_t*>(p + k0) : u32x4_t{0u, 0u, 0u, 0u};
    }
    __device__ __forceinline__ u16x8_t chunk(int c) const {
        const unsigned a = v[2 * c], b = v[2 * c + 1];
        return wq_pack(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, s, false), __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, s, true),
                       __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, s, false), __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, s, true));
    }
};
template <>
struct WqFmt<true> {        // e2m1 codes, two per byte, scl = sc e8m0 [N][K / 32]: one load is one scale block
    static constexpr int LPR = 2, CPL = 4;
    const uint8_t* p;
    const uint8_t* ps;
    unsigned e;             // the block's scale byte
    u32x4_t v;
    __device__ __forceinline__ void init(const uint8_t* q, const void* scl, long row, int part, int K) {
        p = q + row * (K >> 1) + part * 16;
        ps = static_cast<const uint8_t*>(scl) + row * (K >> 5) + part;
    }
    __device__ __forceinline__ void load(int k0, bool in) {
        v = in ? *reinterpret_cast<const u32x4_t*>(p + (k0 >> 1)) : u32x4_t{0u, 0u, 0u, 0u};
        e = in ? ps[k0 >> 5] : 127u;
    }
    __device__ __forceinline__ u16x8_t chunk(int c) const {
        const float s = __uint_as_float(e << 23);
        const unsigned a = v[c];
        return wq_pack(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, s, 0), __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, s, 1),
                       __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, s, 2), __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, s, 3));
    }
};

// v = acc; bias; GELU of the bf16-rounded v; res; round to nearest even: four columns n .. n + 3 of row m
__device__ __forceinline__ void wq_epilogue(const f32x4_t& acc, long m, int n, bf16_t* __restrict__ out, long ldc,
                                            const float* __restrict__ bias, int act, const bf16_t* __restrict__ res) {
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = acc[j];
    if (bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += bias[n + j];     // scalar loads: a bias inside a flat arena is 4-byte aligned
    }
    if (act == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = gelu_tanh(bf2f(f2bf(o[j])));
    }
    if (res) {
        const u16x4_t rr = *reinterpret_cast<const u16x4_t*>(res + m * ldc + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += bf2f(rr[j]);
    }
    *reinterpret_cast<uint2*>(out + m * ldc + n) = uint2{pk2bf(o[0], o[1]), pk2bf(o[2], o[3])};
}

template <int BT, bool FP4>
__global__ void __launch_bounds__(WQ_NT, 2) gemm_wq_kernel(const bf16_t* __restrict__ x, long ldx,
                                                           const uint8_t* __restrict__ q, const void* __restrict__ scl,
                                                           bf16_t* __restrict__ out, long ldc, int M, int N, int K,
                                                           int tiles_m, const float* __restrict__ bias, int act,
                                                           const bf16_t* __restrict__ res) {
    using Fmt = WqFmt<FP4>;
    constexpr int LPR = Fmt::LPR, CPL = Fmt::CPL;
    constexpr int NLOADS = BT * LPR;                        // weight loads of a block and k-step
    constexpr int NL = (NLOADS + WQ_NT - 1) / WQ_NT;        // per lane
    constexpr int NX = BT * 8 / WQ_NT;                      // 16-byte x loads per lane and k-step
    constexpr int FT = BT / 32;                             // 16 x 16 fragments of a wave, each way
    constexpr int IMG = BT * BK;                            // elements of one image
    __shared__ __attribute__((aligned(16))) bf16_t lds[2][2][IMG];      // [buffer][0: dq, 1: x]

    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4, wm = wv & 1, wn = wv >> 1;
    // consecutive blocks share a weight tile and walk the row tiles of x
    const int m0 = (int)(blockIdx.x % tiles_m) * BT, n0 = (int)(blockIdx.x / tiles_m) * BT;

    Fmt w[NL];
    int wko[NL], wlo[NL];       // first element of the lane's load inside a step; its first chunk's image row and chunk
    bool won[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int i = tid + WQ_NT * j, lrow = i / LPR, part = i % LPR;
        won[j] = NLOADS % WQ_NT == 0 || i < NLOADS;         // (64 x 64, fp4: 128 loads, waves 0 and 1)
        wko[j] = part * (BK / LPR);
        wlo[j] = lrow * 8 + part * CPL;                     // row * 8 + chunk
        w[j].init(q, scl, min(n0 + (won[j] ? lrow : 0), N - 1), part, K);
    }
    const bf16_t* xp[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        const int i = tid + WQ_NT * j;                      // image row i >> 3, chunk i & 7
        xp[j] = x + (long)min(m0 + (i >> 3), M - 1) * ldx + (i & 7) * 8;
    }
    u16x8_t xr[NX];

    auto load = [&](int k0) {
#pragma unroll
        for (int j = 0; j < NL; ++j)
            if (won[j]) w[j].load(k0, k0 + wko[j] < K);
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const int i = tid + WQ_NT * j;
            xr[j] = k0 + (i & 7) * 8 < K ? *reinterpret_cast<const u16x8_t*>(xp[j] + k0) : u16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
        }
    };
    auto put_w = [&](int b) {                               // convert and write: what reaches LDS is dq
#pragma unroll
        for (int j = 0; j < NL; ++j)
            if (won[j]) {
#pragma unroll
                for (int c = 0; c < CPL; ++c)
                    *reinterpret_cast<u16x8_t*>(&lds[b][0][kimg_off(wlo[j] >> 3, (wlo[j] & 7) + c)]) = w[j].chunk(c);
            }
    };
    auto put_x = [&](int b) {
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const int i = tid + WQ_NT * j;
            *reinterpret_cast<u16x8_t*>(&lds[b][1][kimg_off(i >> 3, i & 7)]) = xr[j];
        }
    };

    f32x4_t acc[FT][FT];        // [weight fragment][x fragment]
#pragma unroll
    for (int a = 0; a < FT; ++a)
#pragma unroll
        for (int t = 0; t < FT; ++t) acc[a][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto mma = [&](int b, int ks) {                         // the 32 reduction elements ks of buffer b
        bf16x8_t fw[FT], fx[FT];
#pragma unroll
        for (int a = 0; a < FT; ++a) fw[a] = frag_kmajor(lds[b][0], wn * (BT / 2) + a * 16 + r, ks, lane);
#pragma unroll
        for (int t = 0; t < FT; ++t) fx[t] = frag_kmajor(lds[b][1], wm * (BT / 2) + t * 16 + r, ks, lane);
#pragma unroll
        for (int a = 0; a < FT; ++a)
#pragma unroll
            for (int t = 0; t < FT; ++t) acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[a], fx[t], acc[a][t], 0, 0, 0);
    };

    load(0);
    put_w(0);
    put_x(0);
    __syncthreads();
    for (int k0 = 0, b = 0; k0 < K; k0 += BK, b ^= 1) {
        const bool more = k0 + BK < K;                      // block-uniform
        if (more) load(k0 + BK);
        mma(b, 0);
        if (more) put_w(b ^ 1);     // buffer b ^ 1 was last read before the barrier that ended the step before
        mma(b, 1);
        if (more) put_x(b ^ 1);
        __syncthreads();
    }

#pragma unroll
    for (int t = 0; t < FT; ++t) {
        const int m = m0 + wm * (BT / 2) + t * 16 + r;
#pragma unroll
        for (int a = 0; a < FT; ++a) {
            const int n = n0 + wn * (BT / 2) + a * 16 + g * 4;
            if (m < M && n < N) wq_epilogue(acc[a][t], m, n, out, ldc, bias, act, res);
        }
    }
}

template <bool FP4>
int wq_launch(const bf16_t* x, long ldx, const uint8_t* q, const void* scl, bf16_t* out, long ldc, int M, int N, int K,
              const float* bias, int act, const bf16_t* res, int tile, hipStream_t st) {
    constexpr int G = FP4 ? 32 : 16;
    if (!x || !q || !scl || !out || M < 1 || K < G || N < 8 || K % G || N % 8 || (act != 0 && act != 2) || ldx < K ||
        ldc < N || ldx % 8 || ldc % 4 || (tile != 0 && tile != 64 && tile != 128))
        return (int)hipErrorInvalidValue;
    const int bt = tile ? tile : wq_tile(M, N);
    const long tm = cdiv(M, bt), blocks = tm * cdiv(N, bt);
    if (blocks > 0x7FFFFFFFL) return (int)hipErrorInvalidValue;
    if (bt == 128)
        hipLaunchKernelGGL((gemm_wq_kernel<128, FP4>), dim3((unsigned)blocks), dim3(WQ_NT), 0, st, x, ldx, q, scl, out, ldc, M,
                           N, K, (int)tm, bias, act, res);
    else
        hipLaunchKernelGGL((gemm_wq_kernel<64, FP4>), dim3((unsigned)blocks), dim3(WQ_NT), 0, st, x, ldx, q, scl, out, ldc, M, N,
                           K, (int)tm, bias, act, res);
    PDNN_LAUNCH_RET;
}

}  // namespace

// the tile (128 or 64) pdnn_gemm_wq_fp8 / _fp4 run an [M][N] output on; 0 on shapes they do not take
PDNN_API int pdnn_gemm_wq_plan(int M, int N) {
    if (M < 1 || N < 8 || N % 8) return 0;
    return wq_tile(M, N);
}

// x bf16 [M][K] (row stride ldx), q e4m3fn [N][K] contiguous, inv fp32 [N], out bf16 [M][N] (row stride ldc), bias fp32
// [N] or null, res bf16 with out's strides or null, act 0 / 2 (GELU); any M >= 1, K % 16 == 0, N % 8 == 0.  tile: 0 = the
// rule of pdnn_gemm_wq_plan, 64 or 128 for the measuring tools and the tests (the result's bits do not depend on it).
// Non-zero, and nothing launched, for every other argument.
PDNN_API int pdnn_gemm_wq_fp8_tile(const bf16_t* x, long ldx, const uint8_t* q, const float* inv, bf16_t* out, long ldc,
                                   int M, int N, int K, const float* bias, int act, const bf16_t* res, int tile,
                                   hipStream_t st) {
    return wq_launch<false>(x, ldx, q, inv, out, ldc, M, N, K, bias, act, res, tile, st);
}
PDNN_API int pdnn_gemm_wq_fp8(const bf16_t* x, long ldx, const uint8_t* q, const float* inv, bf16_t* out, long ldc, int M,
                              int N, int K, const float* bias, int act, const bf16_t* res, hipStream_t st) {
    return wq_launch<false>(x, ldx, q, inv, out, ldc, M, N, K, bias, act, res, 0, st);
}

// the same on MXFP4: q e2m1 [N][K / 2] and sc e8m0 [N][K / 32] contiguous, K % 32 == 0
PDNN_API int pdnn_gemm_wq_fp4_tile(const bf16_t* x, long ldx, const uint8_t* q, const uint8_t* sc, bf16_t* out, long ldc,
                                   int M, int N, int K, const float* bias, int act, const bf16_t* res, int tile,
                                   hipStream_t st) {
    return wq_launch<true>(x, ldx, q, sc, out, ldc, M, N, K, bias, act, res, tile, st);
}
PDNN_API int pdnn_gemm_wq_fp4(const bf16_t* x, long ldx, const uint8_t* q, const uint8_t* sc, bf16_t* out, long ldc, int M,
                              int N, int K, const float* bias, int act, const bf16_t* res, hipStream_t st) {
    return wq_launch<true>(x, ldx, q, sc, out, ldc, M, N, K, bias, act, res, 0, st);
}
