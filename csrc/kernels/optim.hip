// Fused optimizers and gradient-bucket kernels over FLAT fp32 buffers
// (SURVEY.md §2.8 K-13 gradient accumulate, K-14 average + SGD/Adam update, K-15 bucket
// flatten/scale; reference: pytorch_code/sync_replicas_master_nn.py:22-28,212-219 (avg + SGD),
// MPI_code/src/distributed/sync_replicas_master_nn.h:124-128 (ApplyGrad(lr/count)),
// distributed_TF/src/distributed_train.py:160 (Adam), data_parallel_dist.py:247-263 (flatten, /=world)).
//
// The framework keeps every parameter of a model in ONE contiguous fp32 master buffer and every
// gradient in one contiguous fp32 buffer (DDP buckets are views into it), so an optimizer step is a
// single launch over millions of elements instead of a per-tensor loop.  The same pass refreshes the
// bf16 compute shadow of the weights that the MFMA kernels read, and folds the gradient averaging
// factor (1/world, or 1/alive-count for k-of-n straggler mode) in as `gscale` read from device memory.
#include "common.h"
#include "optim_update.h"

//
// Graph replay: a captured hipGraph bakes kernel arguments in, so the per-step hyper-parameters that
// change between replays (learning rate, Adam's bias corrections) can instead be read from a small
// device buffer `hyper` that the host refreshes (stream-ordered H2D copy) before each replay:
//   SGD:  hyper[0] = lr               Adam: hyper[0] = lr, hyper[1] = 1 - b1^t, hyper[2] = 1 - b2^t
// hyper == nullptr keeps the by-value arguments (eager mode).
namespace {
constexpr int NT = 256;

__global__ void __launch_bounds__(NT) sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                 float* __restrict__ buf, bf16_t* __restrict__ shadow, long n,
                                                 float lr, float momentum, float dampening, float wd,
                                                 int nesterov, const float* __restrict__ gscale_ptr,
                                                 float gscale, int first, const float* __restrict__ hyper) {
    const float gs = gscale_ptr ? gscale * (*gscale_ptr) : gscale;
    if (hyper) lr = hyper[0];
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float pa[4] = {pv.x, pv.y, pv.z, pv.w};
        const float ga[4] = {gv.x, gv.y, gv.z, gv.w};
        float ba[4] = {0, 0, 0, 0};
        if (momentum != 0.f && !first) {
            const float4 bv = reinterpret_cast<float4*>(buf)[i];
            ba[0] = bv.x; ba[1] = bv.y; ba[2] = bv.z; ba[3] = bv.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = sgd_momentum(ga[j] * gs + wd * pa[j], ba[j], momentum, dampening, nesterov, first);
            pa[j] -= lr * d;
        }
        reinterpret_cast<float4*>(p)[i] = make_float4(pa[0], pa[1], pa[2], pa[3]);
        if (momentum != 0.f) reinterpret_cast<float4*>(buf)[i] = make_float4(ba[0], ba[1], ba[2], ba[3]);
        if (shadow) {
            u16x4_t s = {f2bf(pa[0]), f2bf(pa[1]), f2bf(pa[2]), f2bf(pa[3])};
            reinterpret_cast<u16x4_t*>(shadow)[i] = s;
        }
    }
    // tail
    for (long i = n4 * 4 + (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        float d = g[i] * gs + wd * p[i];
        if (momentum != 0.f) {
            float b = first ? 0.f : buf[i];
            d = sgd_momentum(d, b, momentum, dampening, nesterov, first);
            buf[i] = b;
        }
        p[i] -= lr * d;
        if (shadow) shadow[i] = f2bf(p[i]);
    }
}

// Adam / AdamW (decoupled=1).  bc1 = 1 - beta1^t, bc2 = 1 - beta2^t (by value, or hyper[1..2]).
// Memory bound (16 B read + 14 B written per parameter): float4 loads/stores over the 16-B aligned
// body (`vec`, checked by the launcher), scalar tail.
struct AdamCoef {
    float lr, b1, b2, eps, wd, step, rbc2, gs;
    int decoupled;
    __device__ __forceinline__ void upd(float& pi, float gi, float& mi, float& vi) const {
        gi *= gs;
        if (decoupled) pi -= lr * wd * pi;
        else gi += wd * pi;
        adam_moments(gi, mi, vi, b1, b2, 1.f - b1, 1.f - b2);
        pi -= step * mi / adam_denom(vi, rbc2, eps);
    }
};

__global__ void __launch_bounds__(NT) adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ m, float* __restrict__ v,
                                                  bf16_t* __restrict__ shadow, long n, float lr, float b1,
                                                  float b2, float eps, float wd, int decoupled, float bc1,
                                                  float bc2, const float* __restrict__ gscale_ptr,
                                                  float gscale, const float* __restrict__ hyper, int vec) {
    if (hyper) {
        lr = hyper[0];
        bc1 = hyper[1];
        bc2 = hyper[2];
    }
    const AdamCoef c{lr, b1, b2, eps, wd, lr / bc1, rsqrtf(bc2), gscale_ptr ? gscale * (*gscale_ptr) : gscale,
                     decoupled};
    const long n4 = vec ? (n >> 2) : 0;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 mv = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        c.upd(pv.x, gv.x, mv.x, vv.x);
        c.upd(pv.y, gv.y, mv.y, vv.y);
        c.upd(pv.z, gv.z, mv.z, vv.z);
        c.upd(pv.w, gv.w, mv.w, vv.w);
        reinterpret_cast<float4*>(p)[i] = pv;
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(v)[i] = vv;
        if (shadow) {
            u16x4_t s = {f2bf(pv.x), f2bf(pv.y), f2bf(pv.z), f2bf(pv.w)};
            reinterpret_cast<u16x4_t*>(shadow)[i] = s;
        }
    }
    for (long i = n4 * 4 + (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        float pi = p[i], mi = m[i], vi = v[i];
        c.upd(pi, g[i], mi, vi);
        p[i] = pi;
        m[i] = mi;
        v[i] = vi;
        if (shadow) shadow[i] = f2bf(pi);
    }
}

__global__ void __launch_bounds__(NT) cast_f32_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y,
                                                           long n, float scale) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) y[i] = f2bf(x[i] * scale);
}
__global__ void __launch_bounds__(NT) cast_bf16_f32_kernel(const bf16_t* __restrict__ x, float* __restrict__ y,
                                                           long n, float scale, int accumulate) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const float v = bf2f(x[i]) * scale;
        y[i] = accumulate ? y[i] + v : v;
    }
}
__global__ void __launch_bounds__(NT) scale_f32_kernel(float* __restrict__ x, long n, float scale,
                                                       const float* __restrict__ dev_scale, int invert) {
    float s = scale;
    if (dev_scale) s *= invert ? 1.f / fmaxf(*dev_scale, 1.f) : *dev_scale;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) x[i] *= s;
}
// y += a * x  (fp32), used for gradient accumulation of the k-of-n alive-weighted contributions
__global__ void __launch_bounds__(NT) axpy_f32_kernel(float* __restrict__ y, const float* __restrict__ x, long n,
                                                      float a) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) y[i] += a * x[i];
}
// sum of squares (for grad-norm clipping / NaN checks): per-block partial into out[blockIdx]
__global__ void __launch_bounds__(NT) sumsq_kernel(const float* __restrict__ x, long n, float* __restrict__ out) {
    __shared__ float red[NT / 64];
    float s = 0.f;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) s += x[i] * x[i];
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) atomicAdd(out, s);
}

// Global-norm gradient clipping, in two stream-ordered launches that write nothing but a workspace and a 3-float
// result (the gradient itself is only read; the update kernels above apply the coefficient through gscale_ptr).
//
// 1. sumsq_partials_kernel: block b stores the sum of squares of its grid-stride share of g[0, n) to out[b]
//    (every block stores, nothing to zero; no atomics, so the result depends only on n, the alignment of g and
//    the grid).  float4 loads over the 16-byte aligned body, four of them in flight per thread into four
//    accumulators; the <= 3 elements in front of the body and the <= 3 behind it go to block 0's first lanes.
// 2. clip_coef_kernel: one block adds the partials of all ranges in a fixed order in double and writes
//    out[0] = norm of the gradient as the update sees it, out[1] = dev * min(1, max_norm / (norm + 1e-6))
//    (torch.nn.utils.clip_grad_norm_'s formula), out[2] = 1 when the norm is not finite.
constexpr int CLIP_MAX_PARTS = 8 * 512;     // workspace floats: 8 ranges of at most 512 partials (ops/kernels.py)

__device__ __forceinline__ float sq4(const float4 v, float s) {
    return s + ((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w));
}

__global__ void __launch_bounds__(NT) sumsq_partials_kernel(const float* __restrict__ g, long n,
                                                            float* __restrict__ out) {
    __shared__ float red[NT / 64];
    long head = (long)(((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) >> 2);
    if (head > n) head = n;
    const float4* __restrict__ b = reinterpret_cast<const float4*>(g + head);
    const long n4 = (n - head) >> 2;
    const long tail = head + 4 * n4;                   // first element behind the body
    const long stride = (long)gridDim.x * NT;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    long i = (long)blockIdx.x * NT + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const float4 v0 = b[i], v1 = b[i + stride], v2 = b[i + 2 * stride], v3 = b[i + 3 * stride];
        s0 = sq4(v0, s0);
        s1 = sq4(v1, s1);
        s2 = sq4(v2, s2);
        s3 = sq4(v3, s3);
    }
    for (; i < n4; i += stride) s0 = sq4(b[i], s0);
    if (blockIdx.x == 0) {
        const long t = threadIdx.x;
        if (t < head) s1 += g[t] * g[t];
        if (tail + t < n) s2 += g[tail + t] * g[tail + t];
    }
    const float s = block_sum<NT>((s0 + s1) + (s2 + s3), red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__global__ void __launch_bounds__(NT) clip_coef_kernel(const float* __restrict__ partials, int nparts, float max_norm,
                                                       float gscale, const float* __restrict__ dev_scale,
                                                       float* __restrict__ out) {
    __shared__ double red[NT];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += NT) s += (double)partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double dev = dev_scale ? (double)*dev_scale : 1.0;
        const double norm = fabs((double)gscale * dev) * sqrt(red[0]);
        double c = (double)max_norm / (norm + 1e-6);
        c = c > 1.0 ? 1.0 : c;                         // a NaN stays a NaN (torch.clamp(max=1) semantics)
        const float nf = (float)norm;
        out[0] = nf;
        out[1] = (float)(dev * c);
        out[2] = (nf - nf == 0.f) ? 0.f : 1.f;         // inf - inf and NaN - NaN are NaN
    }
}
}  // namespace

PDNN_API int pdnn_sgd_step(float* p, const float* g, float* buf, bf16_t* shadow, long n, float lr, float momentum,
                           float dampening, float wd, int nesterov, const float* gscale_ptr, float gscale, int first,
                           const float* hyper, hipStream_t st) {
    hipLaunchKernelGGL(sgd_kernel, dim3(stream_grid(n / 4 + 1, NT)), dim3(NT), 0, st, p, g, buf, shadow, n, lr,
                       momentum, dampening, wd, nesterov, gscale_ptr, gscale, first, hyper);
    PDNN_LAUNCH_RET;
}

PDNN_API int pdnn_adam_step(float* p, const float* g, float* m, float* v, bf16_t* shadow, long n, float lr, float b1,
                            float b2, float eps, float wd, int decoupled, float bc1, float bc2,
                            const float* gscale_ptr, float gscale, const float* hyper, hipStream_t st) {
    const uintptr_t a16 = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) |
                          reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v);
    const int vec = (a16 & 15) == 0 && (reinterpret_cast<uintptr_t>(shadow) & 7) == 0;
    hipLaunchKernelGGL(adam_kernel, dim3(stream_grid(vec ? n / 4 + 1 : n, NT)), dim3(NT), 0, st, p, g, m, v, shadow,
                       n, lr, b1, b2, eps, wd, decoupled, bc1, bc2, gscale_ptr, gscale, hyper, vec);
    PDNN_LAUNCH_RET;
}

PDNN_API int pdnn_cast_f32_bf16(const float* x, bf16_t* y, long n, float scale, hipStream_t st) {
    hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(stream_grid(n, NT)), dim3(NT), 0, st, x, y, n, scale);
    PDNN_LAUNCH_RET;
}

PDNN_API int pdnn_cast_bf16_f32(const bf16_t* x, float* y, long n, float scale, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3(stream_grid(n, NT)), dim3(NT), 0, st, x, y, n, scale, accumulate);
    PDNN_LAUNCH_RET;
}

PDNN_API int pdnn_scale_f32(float* x, long n, float scale, const float* dev_scale, int invert, hipStream_t st) {
    hipLaunchKernelGGL(scale_f32_kernel, dim3(stream_grid(n, NT)), dim3(NT), 0, st, x, n, scale, dev_scale, invert);
    PDNN_LAUNCH_RET;
}

PDNN_API int pdnn_axpy_f32(float* y, const float* x, long n, float a, hipStream_t st) {
    hipLaunchKernelGGL(axpy_f32_kernel, dim3(stream_grid(n, NT)), dim3(NT), 0, st, y, x, n, a);
    PDNN_LAUNCH_RET;
}

PDNN_API int pdnn_sumsq_f32(const float* x, long n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(sumsq_kernel, dim3(stream_grid(n, NT) > 512 ? 512 : stream_grid(n, NT)), dim3(NT), 0, st, x, n,
                       out);
    PDNN_LAUNCH_RET;
}

// Sum-of-squares partials of g[0, n) into partials[part_off ...]; `partials` is a workspace of CLIP_MAX_PARTS
// floats.  Returns the number of partials written (>= 1; n == 0 writes one 0), or -hipError: nothing is launched
// for a null or misaligned pointer, a negative n, or a part_off whose partials would not fit the workspace.
PDNN_API int pdnn_sumsq_partials(const float* g, long n, float* partials, int part_off, hipStream_t st) {
    if (g == nullptr || partials == nullptr || n < 0 || part_off < 0) return -(int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(partials)) & 3) return -(int)hipErrorInvalidValue;
    const unsigned grid = stream_grid(n / 4 + 1, NT);              // <= 512
    if ((long)part_off + grid > CLIP_MAX_PARTS) return -(int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sumsq_partials_kernel, dim3(grid), dim3(NT), 0, st, g, n, partials + part_off);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? (int)grid : -(int)e;
}

// out[0..2] = {norm, clip coefficient, non-finite flag} from the first nparts workspace partials (see above);
// dev_scale may be null (1).  The update kernels take out + 1 as gscale_ptr.
PDNN_API int pdnn_clip_coef(const float* partials, int nparts, float max_norm, float gscale, const float* dev_scale,
                            float* out, hipStream_t st) {
    if (partials == nullptr || out == nullptr || nparts < 1 || nparts > CLIP_MAX_PARTS)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(NT), 0, st, partials, nparts, max_norm, gscale, dev_scale, out);
    PDNN_LAUNCH_RET;
}
