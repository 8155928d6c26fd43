// Skinny-M weight-streaming GEMM whose x operand is not read from memory: every block produces it into LDS with a
// LayerNorm prologue and then streams its 16 weight rows exactly as gemm_skinny.hip / gemm_skinny_fp8.hip do:
//     x_n = LayerNorm(x) * gamma + beta;      y = act(x_n . w^T + bias)
// for M <= 16 rows (one 16-row MFMA tile) and a reduction length D = the model width, D % 8 == 0 (fp8 weights: % 16),
// D <= 2048 (the LayerNorm kernel's own limit).  A decode block of GPT-2 is then six launches instead of eight (LN1 +
// qkv, attention split and combine, proj, LN2 + fc, fc2).  The rows are cheap enough to be normalised again by every
// block of the grid, so there is no cross-block synchronisation.  (A second prologue, the flash-decoding combine in
// front of proj, and ln_f in front of the 3144-block LM head were built and measured, and lost: profiles/decode_fused.txt.)
//
// One template, two families: <FP8, NW>.  FP8 = false streams bf16 rows w[N][D], FP8 = true e4m3fn codes q[N][D]
// with one power-of-two scale per row (ops/quant.py).  Grid (one block per 16 weight rows), MFMA orientation (16 weight
// rows as A, x as B, v_mfma_f32_16x16x32_bf16), the K partition (NW from pdnn_gemm_skinny_plan /
// pdnn_gemm_skinny_fp8_plan, SL = ceil(units / NW) * unit; no second rule here), the per-wave MFMA order over the
// slice, the wave-order LDS reduction and the epilogue (v = acc; v += bias; GELU of the bf16-rounded v; v += res; RNE)
// are those of the unfused kernels at MT = 1 (res included, though LN1 and LN2 feed GEMMs without one): given the same
// bf16 x image, the output bits are those of gemm_skinny / gemm_skinny_fp8 on that image.  The K tail follows each
// sibling too: bf16 replaces both operands of a 16-byte piece past the slice's end by zero; fp8 replaces the codes by
// +0 and reads x at offset 0 of the row.
//
// Weights first.  A wave issues the nontemporal 16-byte loads of its first weight step (straight to VGPRs) before the
// prologue: they do not depend on x, and the prologue runs under the latency of that first HBM fetch.  One barrier
// sits between prologue and stream.
//
// x image in LDS: bf16 [M][ST], ST = D + 8 if D % 16 == 0 else D + 16 elements, so ST / 8 is odd: the 16 lanes
// r = l & 15 of one g = l >> 4, which read 16 bytes at the same column of rows 0..15, fall into 16 different 16-byte
// bank groups (256 bytes = all 64 banks), the most a ds_read_b128 pass can cover.  The unpadded 2 D-byte stride puts all
// 16 rows on the same banks.  Rows >= M are not read; their fragment is zero.  Dynamic LDS = M * ST * 2 bytes (M = 16,
// D = 2048: 65792 bytes; D = 768: 24832), plus the static reduction buffer of NW KiB.
//
// LN prologue.  Row t is normalised by wave t % NW alone, so a row's bits depend on nothing but the row (not on NW, M
// or the other rows).  A lane owns the 8-element chunks lane + 64 i, as layernorm_fwd_kernel.  Two-pass fp32, written
// with explicit rounding points (contraction off in the function):
//     s   = sum of v, plain adds, chunk order then element order;  mu = wave_sum(s) / D
//     q   = fmaf(v - mu, v - mu, q) in the same order;             rs = rsqrtf(wave_sum(q) / D + eps)
//     out = bf16(fmaf((v - mu) * rs, gamma, beta))
// It is its own model (tested against fp64), not the bits of layernorm_fwd, which is compiled elsewhere with implicit
// contraction.
//
// image (optional): block 0 also stores its LDS image to a bf16 [M][D] buffer (tests); production calls pass null.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no spills, scratch 0 in all 9 instantiations):
//     bf16:  VGPRs 124 (+ 8 AGPRs at NW = 4)    3 - 4 waves / SIMD    static LDS NW KiB (NW = 4, 6, 8, 12)
//     fp8:   VGPRs 140 (+ 8 at NW <= 4)         3                     static LDS NW KiB (NW = 2, 3, 4, 6, 8)
// (the prologue keeps a row's 4 x 8 fp32 values per lane between its passes)
//
// No access leaves w[N][D] (q, inv[N]), x[M][D] (+ ldx), gamma / beta[D], [M][N] (+ ldc), image[M][D]; every entry
// returns non-zero before any launch on arguments outside this.
#include "gemm_common.h"

PDNN_API int pdnn_gemm_skinny_plan(int N, int K);           // gemm_skinny.hip
PDNN_API int pdnn_gemm_skinny_fp8_plan(int N, int K);       // gemm_skinny_fp8.hip

namespace {
using pg::gelu_tanh;

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __bf16 sp_bf2 __attribute__((ext_vector_type(2)));

constexpr int PRO_ROWS = 16;        // rows of x: one MFMA tile
constexpr int PRO_MAXD = 2048;      // model width the image (and the LayerNorm kernel) takes
constexpr int PRO_LNC = PRO_MAXD / 8 / 64;      // 8-element chunks a lane of the LN prologue can own

struct ProArgs {
    const bf16_t* x; long ldx;                  // the prologue: x [M][D], gamma, beta fp32 [D]
    const float *gamma, *beta; float eps;
    const void* w; const float* inv;            // bf16 [N][D], or e4m3fn codes [N][D] and fp32 scales [N]
    bf16_t* out; long ldc;
    int M, N, D, SL, ST;                        // SL: the K slice of a wave, ST: the image's row stride (elements)
    const float* bias; int act;
    const bf16_t* res;
    bf16_t* image;
};

__host__ __device__ constexpr int image_stride(int D) { return D + (D % 16 ? 16 : 8); }

// 8 e4m3 codes (two dwords) of a weight row -> 8 bf16 of dq, exact: sc = the row's inv, a power of two
__device__ __forceinline__ u16x8_t cvt8(unsigned a, unsigned b, float sc) {
    const sp_bf2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, sc, false), p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, sc, true);
    const sp_bf2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, sc, false), p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, sc, true);
    const u32x4_t o = {__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1), __builtin_bit_cast(unsigned, p2),
                       __builtin_bit_cast(unsigned, p3)};
    return __builtin_bit_cast(u16x8_t, o);
}

// rows wv, wv + NW, .. of the image, one wave per row: the arithmetic of the header, every rounding point explicit
template <int NW>
__device__ __forceinline__ void pro_layernorm(const ProArgs& a, bf16_t* img, int wv, int lane) {
#pragma clang fp contract(off)
    const int CH = a.D / 8;
    const float fD = (float)a.D;
    for (int t = wv; t < a.M; t += NW) {
        const bf16_t* xr = a.x + (long)t * a.ldx;
        float v[PRO_LNC][8];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < PRO_LNC; ++i) {
            const int c = lane + 64 * i;
            if (c < CH) {
                unpack8(*reinterpret_cast<const u16x8_t*>(xr + c * 8), v[i]);
#pragma unroll
                for (int j = 0; j < 8; ++j) s += v[i][j];
            }
        }
        const float mu = wave_sum(s) / fD;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < PRO_LNC; ++i) {
            if (lane + 64 * i < CH) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float d = v[i][j] - mu;
                    q = fmaf(d, d, q);
                }
            }
        }
        const float rs = rsqrtf(wave_sum(q) / fD + a.eps);
#pragma unroll
        for (int i = 0; i < PRO_LNC; ++i) {
            const int c = lane + 64 * i;
            if (c < CH) {
                float o[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float n = (v[i][j] - mu) * rs;
                    o[j] = fmaf(n, a.gamma[c * 8 + j], a.beta[c * 8 + j]);
                }
                *reinterpret_cast<u16x8_t*>(img + t * a.ST + c * 8) = pack8(o);
            }
        }
    }
}

template <bool FP8, int NW>
__global__ void __launch_bounds__(NW * 64) gemm_skinny_pro_kernel(const ProArgs a) {
    constexpr int UNIT = FP8 ? 128 : 64;        // reduction elements of one 16-byte load pair
    constexpr int NU = FP8 ? 4 : 2;             // units per step: 8 KiB of weights per wave and 16 rows, as the siblings
    constexpr int NL = 2 * NU;                  // 16-byte weight loads per lane and step
    constexpr int STEP = NU * UNIT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ __attribute__((aligned(16))) f32x4_t red[NW][64];
    bf16_t* img = reinterpret_cast<bf16_t*>(smem);
    const int tid = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int M = a.M, N = a.N, K = a.D;
    const int k0 = min(wv * a.SL, K), k1 = min(k0 + a.SL, K);
    const int nrow = min(n0 + r, N - 1);        // the last group when N % 16 == 8: clamped, its columns never stored
    const char* wrow = reinterpret_cast<const char*>(a.w) + (long)nrow * K * (FP8 ? 1 : 2);
    float sc = 1.f;
    if constexpr (FP8) sc = a.inv[nrow];        // lane r owns weight row n0 + r: its scale rides in the conversion
    const bool mv = r < M;
    const bf16_t* xrow = img + min(r, M - 1) * a.ST;
    const u16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};

    // the weight loads of a step, unmasked (clamped addresses only: offset 0 is in range for every row); the masks
    // are applied where the step is consumed.  bf16: load i = unit i >> 1, elements [16 g + 8 (i & 1), + 8) of it;
    // fp8: elements [32 g + 16 (i & 1), + 16), and a unit wholly past the slice is neither loaded nor consumed
    auto load_w = [&](u32x4_t (&f)[NL], int k) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            if constexpr (FP8) {
                const int ko = k + (i >> 1) * UNIT + g * 32 + (i & 1) * 16;
                if (k + (i >> 1) * UNIT < k1)   // wave-uniform
                    f[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wrow + (ko + 16 <= k1 ? ko : 0)));
            } else {
                const int ko = k + (i >> 1) * UNIT + g * 16 + (i & 1) * 8;
                f[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wrow + 2 * (ko + 8 <= k1 ? ko : 0)));
            }
        }
    };
    auto xfrag = [&](int ko) { return *reinterpret_cast<const u16x8_t*>(xrow + ko); };      // ko + 8 <= D <= ST
    auto mfma = [&](const u16x8_t& wq, const u16x8_t& xq) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wq), __builtin_bit_cast(bf16x8_t, xq),
                                                      acc, 0, 0, 0);
    };
    auto step = [&](const u32x4_t (&f)[NL], int k) {
        if constexpr (FP8) {
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int ku = k + u * UNIT;
                if (ku < k1) {                  // wave-uniform
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const bool kv = ku + g * 32 + (h >> 1) * 16 + 16 <= k1;
                        const u32x4_t& wl = f[2 * u + (h >> 1)];
                        const u16x8_t wq = cvt8(kv ? wl[2 * (h & 1)] : 0u, kv ? wl[2 * (h & 1) + 1] : 0u, sc);
                        const int ko = ku + g * 32 + h * 8;
                        mfma(wq, mv ? xfrag(ko + 8 <= k1 ? ko : 0) : zero);
                    }
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                const int ko = k + (q >> 1) * UNIT + g * 16 + (q & 1) * 8;
                const bool kv = ko + 8 <= k1;
                mfma(kv ? __builtin_bit_cast(u16x8_t, f[q]) : zero, (kv && mv) ? xfrag(ko) : zero);
            }
        }
    };

    u32x4_t fa[NL], fb[NL];
    if (k0 < k1) load_w(fa, k0);                // wave-uniform: the first step is in flight under the prologue
    pro_layernorm<NW>(a, img, wv, lane);
    __syncthreads();
    if (a.image && blockIdx.x == 0) {           // block-uniform
        const int CH = K / 8;
        for (int c = tid; c < M * CH; c += NW * 64) {
            const int row = c / CH, ch = c - row * CH;
            *reinterpret_cast<u16x8_t*>(a.image + (long)row * K + ch * 8) = *reinterpret_cast<const u16x8_t*>(img + row * a.ST + ch * 8);
        }
    }
    if (k0 < k1) {
        int k = k0;
        while (true) {
            if (k + STEP >= k1) {
                step(fa, k);
                break;
            }
            load_w(fb, k + STEP);
            step(fa, k);
            k += STEP;
            if (k + STEP >= k1) {
                step(fb, k);
                break;
            }
            load_w(fa, k + STEP);
            step(fb, k);
            k += STEP;
        }
    }
    red[wv][lane] = acc;
    __syncthreads();
    if (wv != 0) return;                        // wave 0 finishes the one row tile
    f32x4_t v = red[0][lane];
#pragma unroll
    for (int i = 1; i < NW; ++i) v += red[i][lane];
    const int m = r, n = n0 + g * 4;
    if (m >= M || n >= N) return;               // N % 8 == 0: n < N covers n .. n + 3
    float o[4] = {v[0], v[1], v[2], v[3]};
    if (a.bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += a.bias[n + j];  // scalar loads: a bias inside a flat arena is 4-byte aligned
    }
    if (a.act == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = gelu_tanh(bf2f(f2bf(o[j])));
    }
    if (a.res) {
        const u16x4_t rr = *reinterpret_cast<const u16x4_t*>(a.res + (long)m * a.ldc + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += bf2f(rr[j]);
    }
    *reinterpret_cast<uint2*>(a.out + (long)m * a.ldc + n) = uint2{pk2bf(o[0], o[1]), pk2bf(o[2], o[3])};
}

template <bool FP8, int NW>
void pro_launch(const ProArgs& a, hipStream_t st) {
    static bool attr = false;
    if (!attr) {                                // the largest image is past the 64 KiB a launch gets unasked
        attr = true;
        (void)hipFuncSetAttribute((const void*)gemm_skinny_pro_kernel<FP8, NW>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, PRO_ROWS * image_stride(PRO_MAXD) * 2);
    }
    hipLaunchKernelGGL((gemm_skinny_pro_kernel<FP8, NW>), dim3((unsigned)cdiv(a.N, 16)), dim3(NW * 64),
                       (size_t)a.M * a.ST * 2, st, a);
}

bool aligned(const void* p, unsigned n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// the checks, then the partition of the sibling kernel and the launch
template <bool FP8>
int pro_entry(ProArgs a, hipStream_t st) {
    const int dq = FP8 ? 16 : 8;
    if (!a.x || !a.gamma || !a.beta || !a.w || !a.out || (FP8 && !a.inv) || a.M < 1 || a.M > PRO_ROWS || a.N < 8 ||
        a.N % 8 || a.D < dq || a.D % dq || a.D > PRO_MAXD || (a.act != 0 && a.act != 2) || a.ldx < a.D || a.ldx % 8 ||
        a.ldc < a.N || a.ldc % 4 || !aligned(a.x, 16) || !aligned(a.w, 16) || !aligned(a.out, 8) || !aligned(a.image, 16) ||
        !aligned(a.gamma, 4) || !aligned(a.beta, 4) || !aligned(a.bias, 4) || !aligned(a.inv, 4))
        return (int)hipErrorInvalidValue;
    const int nw = FP8 ? pdnn_gemm_skinny_fp8_plan(a.N, a.D) : pdnn_gemm_skinny_plan(a.N, a.D);
    if (nw < 1) return (int)hipErrorInvalidValue;
    const int unit = FP8 ? 128 : 64;
    a.SL = (int)cdiv(cdiv(a.D, unit), nw) * unit;
    a.ST = image_stride(a.D);
    if constexpr (FP8) {
        switch (nw) {
            case 2: pro_launch<true, 2>(a, st); break;
            case 3: pro_launch<true, 3>(a, st); break;
            case 4: pro_launch<true, 4>(a, st); break;
            case 6: pro_launch<true, 6>(a, st); break;
            case 8: pro_launch<true, 8>(a, st); break;
            default: return (int)hipErrorInvalidValue;
        }
    } else {
        switch (nw) {
            case 4: pro_launch<false, 4>(a, st); break;
            case 6: pro_launch<false, 6>(a, st); break;
            case 8: pro_launch<false, 8>(a, st); break;
            case 12: pro_launch<false, 12>(a, st); break;
            default: return (int)hipErrorInvalidValue;
        }
    }
    PDNN_LAUNCH_RET;
}

}  // namespace

// out [M][N] (row stride ldc) = act(LayerNorm(x [M][D], row stride ldx; gamma, beta fp32 [D]; eps) . w [N][D]^T + bias),
// 1 <= M <= 16, D % 8 == 0, 8 <= D <= 2048, N % 8 == 0; act 0 / 2 (GELU); image: null, or bf16 [M][D] that receives the
// normalised rows.  Non-zero, and nothing launched, for every other argument.
PDNN_API int pdnn_gemm_skinny_ln(const bf16_t* x, long ldx, const float* gamma, const float* beta, float eps,
                                 const bf16_t* w, bf16_t* out, long ldc, int M, int N, int D, const float* bias, int act,
                                 bf16_t* image, hipStream_t st) {
    return pro_entry<false>(ProArgs{x, ldx, gamma, beta, eps, w, nullptr, out, ldc, M, N, D, 0, 0, bias, act, nullptr, image}, st);
}

// the same on e4m3fn codes q [N][D] with row scales inv [N] (gemm_skinny_fp8.hip's format); D % 16 == 0
PDNN_API int pdnn_gemm_skinny_ln_fp8(const bf16_t* x, long ldx, const float* gamma, const float* beta, float eps,
                                     const uint8_t* q, const float* inv, bf16_t* out, long ldc, int M, int N, int D,
                                     const float* bias, int act, bf16_t* image, hipStream_t st) {
    return pro_entry<true>(ProArgs{x, ldx, gamma, beta, eps, q, inv, out, ldc, M, N, D, 0, 0, bias, act, nullptr, image}, st);
}
