// Layer-wise optimizers on the flat arena: LARS (SGD under a per-tensor trust ratio) and LAMB (Adam under one).
//
// The flat kernels of optim.hip see one range of floats and one lr / weight decay for all of it.  These kernels
// see SEGMENTS: one parameter's slice [off, off + numel) of the range.  The 64-element alignment padding between
// parameters belongs to no segment: it is never read into a norm and never written, in the weights, the bf16
// shadow or any state buffer.  Two small device tables, built by the host once per param group, describe the range:
//
//   LwSeg   one per parameter: offset, numel, weight decay (0 for an excluded parameter), adapt flag, and the
//           parameter's run [chunk0, chunk0 + nchunks) of the chunk table;
//   LwChunk every segment cut into chunks of at most LW_CHUNK elements: start, segment id, length.
//
// One block works on one chunk, so a 64-element BatchNorm gain and a 38.6M-element embedding both fill the chip.
// A step of one param group is three stream-ordered launches:
//
// 1. lw_norm_kernel, one block per chunk.  LARS: the block stores its chunk's sum of w^2 and of g^2 to
//    partials[2 chunk], partials[2 chunk + 1].  LAMB: the block performs the moment update (reads p, g, m, v,
//    writes m, v), forms u = m^ / (sqrt(v^) + eps) + wd_seg w and stores the sums of w^2 and u^2; p is not written.
//    Every block stores its own slot: no atomics, nothing to zero, the result depends only on the tables.
// 2. lw_ratio_kernel, one block per segment: adds the segment's chunk partials in a fixed order in double (the
//    discipline of optim.hip's clip_coef_kernel) and writes out[seg] = trust ratio, out[nseg + seg] = ||w||,
//    out[2 nseg + seg] = the other norm (LARS: |gs| ||g||, the gradient as the update sees it; LAMB: ||u||).
//      LARS  r = eta ||w|| / (|gs| ||g|| + wd_seg ||w|| + eps)        LAMB  r = ||w|| / ||u||
//    r = 1 when the segment is not adapted, when ||w|| is 0 or when the other norm is 0; clamp: r = min(r, 1).
// 3. lw_lars_apply_kernel / lw_lamb_apply_kernel, one block per chunk.  LARS: d = r (gs g + wd_seg w), then SGD's
//    momentum / dampening / Nesterov / first-step recurrence on d (optim_update.h), then p -= lr (...).  LAMB:
//    u again from the stored m and v, p -= lr r u.  Both refresh the bf16 shadow in the same pass.
//
// gs = gscale * (*gscale_ptr) is the factor the flat update kernels apply: the clip coefficient and the 1/alive
// scale fold in exactly as they do there.  hyper[] is the graph-replay contract of optim.hip: hyper[0] = lr, and
// for LAMB hyper[1] = 1 - b1^t, hyper[2] = 1 - b2^t.
//
// Inside a chunk: float4 accesses over the 16-byte aligned body, scalar head (<= 3) and tail (<= 3).  The entry
// points require 16-byte aligned base pointers, so a chunk's body is aligned whatever its start.  The kernels trust
// the tables; ops/kernels.py checks them on the host before they are uploaded.
#include "common.h"
#include "optim_update.h"

namespace {
constexpr int NT = 256;
constexpr int LW_CHUNK = 16384;      // elements per chunk (ops/kernels.py LW_CHUNK): 16 float4 per thread

struct LwSeg {
    long off, numel;
    float wd;
    int adapt, chunk0, nchunks;
};
struct LwChunk {
    long start;
    int seg, len;
};
static_assert(sizeof(LwSeg) == 32 && sizeof(LwChunk) == 16, "table layouts are mirrored in ops/kernels.py");

// Visit the chunk [start, start + len) of a 16-byte aligned base: body4(i) for every aligned group of four
// elements i .. i + 3, body1(i) for the <= 3 elements in front of the body and the <= 3 behind it.
template <int UNROLL, class F4, class F1>
__device__ __forceinline__ void chunk_for(long start, int len, F4 body4, F1 body1) {
    int head = (int)((4 - (start & 3)) & 3);
    if (head > len) head = len;
    const int n4 = (len - head) >> 2, tail = head + 4 * n4, t = threadIdx.x;
    const long b = start + head;
#pragma unroll UNROLL
    for (int i = t; i < n4; i += NT) body4(b + 4L * i);
    if (t < head) body1(start + t);
    if (tail + t < len) body1(start + tail + t);
}

__device__ __forceinline__ float4 ld4(const float* p, long i) { return *reinterpret_cast<const float4*>(p + i); }
__device__ __forceinline__ void st4(float* p, long i, float4 v) { *reinterpret_cast<float4*>(p + i) = v; }
__device__ __forceinline__ void st4bf(bf16_t* s, long i, float4 v) {
    const u16x4_t o = {f2bf(v.x), f2bf(v.y), f2bf(v.z), f2bf(v.w)};
    *reinterpret_cast<u16x4_t*>(s + i) = o;
}
__device__ __forceinline__ float sq4(const float4 v, float s) {
    return s + ((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w));
}

// LAMB's per-element expressions: the moments are Adam's (optim_update.h), u is the bias-corrected Adam direction
// plus the segment's weight decay.
struct LambCoef {
    float b1, b2, c1, c2, eps, rbc1, rbc2, gs, wd;     // c1 = 1 - b1, c2 = 1 - b2, formed in double on the host
    __device__ __forceinline__ float u(float w, float mi, float vi) const {
        return (mi * rbc1) / adam_denom(vi, rbc2, eps) + wd * w;
    }
    __device__ __forceinline__ float moments(float w, float gi, float& mi, float& vi) const {
        adam_moments(gi * gs, mi, vi, b1, b2, c1, c2);
        return u(w, mi, vi);
    }
};

template <int LAMB>
__global__ void __launch_bounds__(NT) lw_norm_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ m, float* __restrict__ v,
                                                     const LwSeg* __restrict__ segs,
                                                     const LwChunk* __restrict__ chunks,
                                                     float* __restrict__ partials, float b1, float b2, float c1,
                                                     float c2, float eps, float bc1, float bc2,
                                                     const float* __restrict__ gscale_ptr,
                                                     float gscale, const float* __restrict__ hyper) {
    __shared__ float red[NT / 64];
    const LwChunk ck = chunks[blockIdx.x];
    float sw = 0.f, su = 0.f;
    if (LAMB) {
        if (hyper) {
            bc1 = hyper[1];
            bc2 = hyper[2];
        }
        const LambCoef c{b1, b2, c1, c2, eps, 1.f / bc1, rsqrtf(bc2), gscale_ptr ? gscale * (*gscale_ptr) : gscale,
                         segs[ck.seg].wd};
        chunk_for<2>(
            ck.start, ck.len,
            [&](long i) {
                const float4 wv = ld4(p, i), gv = ld4(g, i);
                float4 mv = ld4(m, i), vv = ld4(v, i);
                float4 uv;
                uv.x = c.moments(wv.x, gv.x, mv.x, vv.x);
                uv.y = c.moments(wv.y, gv.y, mv.y, vv.y);
                uv.z = c.moments(wv.z, gv.z, mv.z, vv.z);
                uv.w = c.moments(wv.w, gv.w, mv.w, vv.w);
                st4(m, i, mv);
                st4(v, i, vv);
                sw = sq4(wv, sw);
                su = sq4(uv, su);
            },
            [&](long i) {
                const float w = p[i];
                float mi = m[i], vi = v[i];
                const float ui = c.moments(w, g[i], mi, vi);
                m[i] = mi;
                v[i] = vi;
                sw += w * w;
                su += ui * ui;
            });
    } else {
        chunk_for<4>(
            ck.start, ck.len,
            [&](long i) {
                sw = sq4(ld4(p, i), sw);
                su = sq4(ld4(g, i), su);
            },
            [&](long i) {
                sw += p[i] * p[i];
                su += g[i] * g[i];
            });
    }
    sw = block_sum<NT>(sw, red);
    su = block_sum<NT>(su, red);
    if (threadIdx.x == 0) {
        partials[2 * (long)blockIdx.x] = sw;
        partials[2 * (long)blockIdx.x + 1] = su;
    }
}

__global__ void __launch_bounds__(NT) lw_ratio_kernel(const float* __restrict__ partials,
                                                      const LwSeg* __restrict__ segs, int nseg, int lamb, float eta,
                                                      float eps, int clamp, const float* __restrict__ gscale_ptr,
                                                      float gscale, float* __restrict__ out) {
    __shared__ double red[2][NT];
    const LwSeg sg = segs[blockIdx.x];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < sg.nchunks; i += NT) {
        a += (double)partials[2 * (long)(sg.chunk0 + i)];
        b += (double)partials[2 * (long)(sg.chunk0 + i) + 1];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double gs = gscale_ptr ? (double)gscale * (double)*gscale_ptr : (double)gscale;
        const double wn = sqrt(red[0][0]);
        const double un = lamb ? sqrt(red[1][0]) : fabs(gs) * sqrt(red[1][0]);
        double r = 1.0;
        if (sg.adapt && !(wn == 0.0) && !(un == 0.0)) {   // a NaN norm takes the formula and stays a NaN
            r = lamb ? wn / un : (double)eta * wn / (un + (double)sg.wd * wn + (double)eps);
            if (clamp) r = r > 1.0 ? 1.0 : r;
        }
        out[blockIdx.x] = (float)r;
        out[(long)nseg + blockIdx.x] = (float)wn;
        out[2L * nseg + blockIdx.x] = (float)un;
    }
}

__global__ void __launch_bounds__(NT) lw_lars_apply_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ buf, bf16_t* __restrict__ shadow,
                                                           const LwSeg* __restrict__ segs,
                                                           const LwChunk* __restrict__ chunks,
                                                           const float* __restrict__ ratio, float lr, float momentum,
                                                           float dampening, int nesterov, int first,
                                                           const float* __restrict__ gscale_ptr, float gscale,
                                                           const float* __restrict__ hyper) {
    const LwChunk ck = chunks[blockIdx.x];
    const float gs = gscale_ptr ? gscale * (*gscale_ptr) : gscale;
    if (hyper) lr = hyper[0];
    const float r = ratio[ck.seg], wd = segs[ck.seg].wd;
    const bool mom = momentum != 0.f;
    auto upd = [&](float& w, float gi, float& b) {
        const float d = sgd_momentum(r * (gs * gi + wd * w), b, momentum, dampening, nesterov, first);
        w -= lr * d;
    };
    chunk_for<2>(
        ck.start, ck.len,
        [&](long i) {
            float4 wv = ld4(p, i);
            const float4 gv = ld4(g, i);
            float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (mom && !first) bv = ld4(buf, i);
            upd(wv.x, gv.x, bv.x);
            upd(wv.y, gv.y, bv.y);
            upd(wv.z, gv.z, bv.z);
            upd(wv.w, gv.w, bv.w);
            st4(p, i, wv);
            if (mom) st4(buf, i, bv);
            if (shadow) st4bf(shadow, i, wv);
        },
        [&](long i) {
            float w = p[i], b = (mom && !first) ? buf[i] : 0.f;
            upd(w, g[i], b);
            p[i] = w;
            if (mom) buf[i] = b;
            if (shadow) shadow[i] = f2bf(w);
        });
}

__global__ void __launch_bounds__(NT) lw_lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                           const float* __restrict__ v, bf16_t* __restrict__ shadow,
                                                           const LwSeg* __restrict__ segs,
                                                           const LwChunk* __restrict__ chunks,
                                                           const float* __restrict__ ratio, float lr, float eps,
                                                           float bc1, float bc2, const float* __restrict__ hyper) {
    const LwChunk ck = chunks[blockIdx.x];
    if (hyper) {
        lr = hyper[0];
        bc1 = hyper[1];
        bc2 = hyper[2];
    }
    const LambCoef c{0.f, 0.f, 0.f, 0.f, eps, 1.f / bc1, rsqrtf(bc2), 1.f, segs[ck.seg].wd};
    const float step = lr * ratio[ck.seg];
    chunk_for<2>(
        ck.start, ck.len,
        [&](long i) {
            float4 wv = ld4(p, i);
            const float4 mv = ld4(m, i), vv = ld4(v, i);
            wv.x -= step * c.u(wv.x, mv.x, vv.x);
            wv.y -= step * c.u(wv.y, mv.y, vv.y);
            wv.z -= step * c.u(wv.z, mv.z, vv.z);
            wv.w -= step * c.u(wv.w, mv.w, vv.w);
            st4(p, i, wv);
            if (shadow) st4bf(shadow, i, wv);
        },
        [&](long i) {
            float w = p[i];
            w -= step * c.u(w, m[i], v[i]);
            p[i] = w;
            if (shadow) shadow[i] = f2bf(w);
        });
}

inline bool a16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
inline bool tables_ok(const void* segs, const void* chunks, int nseg, int nchunk) {
    return segs != nullptr && chunks != nullptr && a16(segs) && a16(chunks) && nseg >= 1 && nchunk >= nseg;
}
}  // namespace

PDNN_API int pdnn_lw_chunk() { return LW_CHUNK; }

// Entry points.  Each returns hipErrorInvalidValue and launches nothing for a null pointer, a base pointer that is
// not 16-byte aligned (8 for the bf16 shadow, which may be null: no shadow), nseg < 1 or nchunk < nseg.

// partials[0, 2 nchunk) = per chunk {sum w^2, sum g^2} (lamb == 0; m and v unused) or, after the moment update of
// m and v, {sum w^2, sum u^2} (lamb == 1); c1 = 1 - b1, c2 = 1 - b2, taken in double by the caller.
PDNN_API int pdnn_lw_norm_partials(const float* p, const float* g, float* m, float* v, const void* segs,
                                   const void* chunks, int nseg, int nchunk, float* partials, int lamb, float b1,
                                   float b2, float c1, float c2, float eps, float bc1, float bc2,
                                   const float* gscale_ptr, float gscale, const float* hyper, hipStream_t st) {
    if (p == nullptr || g == nullptr || partials == nullptr || !tables_ok(segs, chunks, nseg, nchunk))
        return (int)hipErrorInvalidValue;
    if (!a16(p) || !a16(g) || !a16(partials)) return (int)hipErrorInvalidValue;
    if (lamb && (m == nullptr || v == nullptr || !a16(m) || !a16(v))) return (int)hipErrorInvalidValue;
    const LwSeg* sg = static_cast<const LwSeg*>(segs);
    const LwChunk* ck = static_cast<const LwChunk*>(chunks);
    if (lamb)
        hipLaunchKernelGGL(lw_norm_kernel<1>, dim3(nchunk), dim3(NT), 0, st, p, g, m, v, sg, ck, partials, b1, b2,
                           c1, c2, eps, bc1, bc2, gscale_ptr, gscale, hyper);
    else
        hipLaunchKernelGGL(lw_norm_kernel<0>, dim3(nchunk), dim3(NT), 0, st, p, g, m, v, sg, ck, partials, b1, b2,
                           c1, c2, eps, bc1, bc2, gscale_ptr, gscale, hyper);
    PDNN_LAUNCH_RET;
}

// out[0, nseg) = trust ratios, out[nseg, 2 nseg) = ||w||, out[2 nseg, 3 nseg) = the other norm, from the chunk
// partials of pdnn_lw_norm_partials.
PDNN_API int pdnn_lw_ratio(const float* partials, const void* segs, int nseg, int nchunk, int lamb, float eta,
                           float eps, int clamp, const float* gscale_ptr, float gscale, float* out, hipStream_t st) {
    if (partials == nullptr || out == nullptr || segs == nullptr || !a16(segs) || nseg < 1 || nchunk < nseg)
        return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(partials) | reinterpret_cast<uintptr_t>(out)) & 3)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lw_ratio_kernel, dim3(nseg), dim3(NT), 0, st, partials, static_cast<const LwSeg*>(segs), nseg,
                       lamb, eta, eps, clamp, gscale_ptr, gscale, out);
    PDNN_LAUNCH_RET;
}

PDNN_API int pdnn_lars_apply(float* p, const float* g, float* buf, bf16_t* shadow, const void* segs,
                             const void* chunks, int nseg, int nchunk, const float* ratio, float lr, float momentum,
                             float dampening, int nesterov, int first, const float* gscale_ptr, float gscale,
                             const float* hyper, hipStream_t st) {
    if (p == nullptr || g == nullptr || ratio == nullptr || !tables_ok(segs, chunks, nseg, nchunk))
        return (int)hipErrorInvalidValue;
    if (!a16(p) || !a16(g) || (reinterpret_cast<uintptr_t>(shadow) & 7)) return (int)hipErrorInvalidValue;
    if (momentum != 0.f && (buf == nullptr || !a16(buf))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lw_lars_apply_kernel, dim3(nchunk), dim3(NT), 0, st, p, g, buf, shadow,
                       static_cast<const LwSeg*>(segs), static_cast<const LwChunk*>(chunks), ratio, lr, momentum,
                       dampening, nesterov, first, gscale_ptr, gscale, hyper);
    PDNN_LAUNCH_RET;
}

PDNN_API int pdnn_lamb_apply(float* p, const float* m, const float* v, bf16_t* shadow, const void* segs,
                             const void* chunks, int nseg, int nchunk, const float* ratio, float lr, float eps,
                             float bc1, float bc2, const float* hyper, hipStream_t st) {
    if (p == nullptr || m == nullptr || v == nullptr || ratio == nullptr || !tables_ok(segs, chunks, nseg, nchunk))
        return (int)hipErrorInvalidValue;
    if (!a16(p) || !a16(m) || !a16(v) || (reinterpret_cast<uintptr_t>(shadow) & 7))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lw_lamb_apply_kernel, dim3(nchunk), dim3(NT), 0, st, p, m, v, shadow,
                       static_cast<const LwSeg*>(segs), static_cast<const LwChunk*>(chunks), ratio, lr, eps, bc1, bc2,
                       hyper);
    PDNN_LAUNCH_RET;
}
