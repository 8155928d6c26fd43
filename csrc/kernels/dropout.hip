// Dropout on bf16 rows [R][D] (the residual adds and the embedding of GPT-2), and the export of the generator's keep
// bits for tests and for the CPU path's parity.  The generator is dropout_rng.h: nothing is stored, the backward kernel
// derives the bits the forward used from the same (state, site).  D % 8 == 0, 16-byte accesses: one thread per 8
// columns = two words of the generator (granule idx 2 c and 2 c + 1 of chunk c, since D / 4 = 2 (D / 8)).
#include "common.h"
#include "dropout_rng.h"

namespace {
constexpr int NT = 256;

// y = res + keep o x * scale (RES), y = keep o x * scale (!RES).  y may alias x: a thread reads its chunk before it
// writes it, and no other thread touches that chunk
template <bool RES>
__global__ void __launch_bounds__(NT) dropout_rows_kernel(const bf16_t* x, const bf16_t* res, bf16_t* y, long nchunk,
                                                          pdrop::Arg a) {
    const pdrop::Key k = pdrop::stream_key(a.state, a.site, 0u);
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < nchunk; c += (long)gridDim.x * NT) {
        float f[8], r[8];
        unpack8(*reinterpret_cast<const u16x8_t*>(x + 8 * c), f);
        if constexpr (RES) unpack8(*reinterpret_cast<const u16x8_t*>(res + 8 * c), r);
        const uint32_t w0 = pdrop::word(k, (uint32_t)(2 * c)), w1 = pdrop::word(k, (uint32_t)(2 * c + 1));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = pdrop::keep(j < 4 ? w0 : w1, j & 3, a.thr) ? f[j] * a.scale : 0.f;
            f[j] = RES ? r[j] + v : v;
        }
        *reinterpret_cast<u16x8_t*>(y + 8 * c) = pack8(f);
    }
}

// keep bytes (1 = kept) of nw words per stream: rows have one stream, attention B * H of T * T / 4 words each
__global__ void __launch_bounds__(NT) dropout_mask_kernel(uint32_t* out, long nw, long total, pdrop::Arg a) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const long stream = i / nw;
        const pdrop::Key k = pdrop::stream_key(a.state, a.site, (uint32_t)stream);
        const uint32_t w = pdrop::word(k, (uint32_t)(i - stream * nw));
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) v |= (pdrop::keep(w, j, a.thr) ? 1u : 0u) << (8 * j);
        out[i] = v;
    }
}

bool rows_arg(float p, const long long* state, int site, long R, int D, pdrop::Arg* a) {
    uint32_t thr;
    if (!pdrop::threshold(p, &thr) || !state || site < 0 || R < 1 || D < 8 || D % 8 || R * (long)(D / 4) > (1L << 32))
        return false;
    *a = pdrop::Arg{state, (uint32_t)site, thr, pdrop::scale_of(thr)};
    return true;
}
}  // namespace

// the quantised probability thr / 256 that p stands for; -1 for p outside [0, 1)
PDNN_API float pdnn_dropout_p_eff(float p) {
    uint32_t thr;
    return pdrop::threshold(p, &thr) ? (float)thr / 256.f : -1.f;
}

// y = res + keep o x / (1 - p_eff); res may be null, y may be x
PDNN_API int pdnn_dropout_add_fwd(const bf16_t* x, const bf16_t* res, bf16_t* y, long R, int D, float p,
                                  const long long* state, int site, hipStream_t st) {
    pdrop::Arg a;
    if (!x || !y || !rows_arg(p, state, site, R, D, &a)) return (int)hipErrorInvalidValue;
    const long nchunk = R * (D / 8);
    if (res)
        hipLaunchKernelGGL(dropout_rows_kernel<true>, dim3(stream_grid(nchunk, NT)), dim3(NT), 0, st, x, res, y, nchunk, a);
    else
        hipLaunchKernelGGL(dropout_rows_kernel<false>, dim3(stream_grid(nchunk, NT)), dim3(NT), 0, st, x, res, y, nchunk, a);
    PDNN_LAUNCH_RET;
}

// dx = keep o g / (1 - p_eff): the same bits as the forward of (state, site)
PDNN_API int pdnn_dropout_bwd(const bf16_t* g, bf16_t* dx, long R, int D, float p, const long long* state, int site,
                              hipStream_t st) {
    return pdnn_dropout_add_fwd(g, nullptr, dx, R, D, p, state, site, st);
}

// out uint8 [R][D]: 1 where (row, col) is kept
PDNN_API int pdnn_dropout_mask_rows(uint8_t* out, long R, int D, float p, const long long* state, int site,
                                    hipStream_t st) {
    pdrop::Arg a;
    if (!out || !rows_arg(p, state, site, R, D, &a)) return (int)hipErrorInvalidValue;
    const long nw = R * (D / 4);
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(stream_grid(nw, NT)), dim3(NT), 0, st, reinterpret_cast<uint32_t*>(out), nw,
                       nw, a);
    PDNN_LAUNCH_RET;
}

// out uint8 [B][H][T(q)][T(k)]: 1 where the probability of (b, h, q, k) is kept
PDNN_API int pdnn_dropout_mask_attn(uint8_t* out, int B, int H, int T, float p, const long long* state, int site,
                                    hipStream_t st) {
    uint32_t thr;
    if (!out || !pdrop::threshold(p, &thr) || !state || site < 0 || B < 1 || H < 1 || T < 4 || T % 4 || T > 65536)
        return (int)hipErrorInvalidValue;
    const pdrop::Arg a{state, (uint32_t)site, thr, pdrop::scale_of(thr)};
    const long nw = (long)T * (T / 4);
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(stream_grid(nw * B * H, NT)), dim3(NT), 0, st,
                       reinterpret_cast<uint32_t*>(out), nw, nw * B * H, a);
    PDNN_LAUNCH_RET;
}
