// Token sampling for the decode loop: one launch per step takes the logits row of every sequence, applies temperature,
// top-k, top-p and the eos mask, draws from the counter-based generator of dropout_rng.h and writes the token where the
// next step's embedding_decode reads it.  ops/sampling.py sample_reference (torch, fp64 weights) and tests/sample_ref.py
// (numpy, fp64) implement the same definition.
//
// Definition of a draw.  Row b: logits l[0..V) (NaN counts as -inf, -0 as +0), temperature T >= 0, optional k >= 1,
// optional p, a uniform u in [0, 1).  T and p are fp32 values.
//   greedy    T == 0: the smallest index holding the maximum value.  No random number is used.
//   top-k     decided on the raw logit values, before any arithmetic, so it is exact.  If k < V, t_k is the k-th
//             largest value counted with multiplicity and the kept set is {i : l_i >= t_k}: ties at the threshold are
//             all kept.  k >= V or none keeps everything.
//   weights   w_i = exp((l_i - m) / T) on the kept set, m the row maximum; w_i = 0 elsewhere, and for -inf.
//   top-p     applies when 0 < p < 1 (none, or p >= 1: no filter).  W_k is the sum of the kept weights; t_p is the largest
//             value v among the kept logits with sum_{l_i >= v} w_i >= p W_k; the final set is S = {i kept : l_i >= t_p}.
//             Ties are kept whole and the maximum is always in S.
//   draw      W = sum_S w_i.  The token is the smallest i in S, in ascending token index, with
//             sum_{j in S, j <= i} w_j > u W; if rounding leaves no such i, the largest i in S with w_i > 0.
//   degenerate  a row with no finite logit yields token 0.  +inf logits are unsupported.
//   eos       with an eos id and a finished byte per row, a finished row gets eos and draws nothing; afterwards
//             finished[b] |= (token == eos).
//   u         key = pdrop::stream_key(state, SITE_SAMPLE, stream = b), state int64[2] = (seed, step) read from device
//             memory (a replayed graph sees the current step); u = (word(key, 0) >> 8) * 2^-24, exact in fp32.  An
//             optional fp32 [B] override replaces it (clamped to [0, 1 - 2^-24], truncated to a multiple of 2^-24).
//   aux       thr[b] = max(t_k, t_p) with an absent filter counting as -inf (the smallest value a member of S may have),
//             nkeep[b] = #{i : l_i >= thr[b]}.  Greedy: thr = m, nkeep = 1.  No finite logit: thr = -inf, nkeep = 0.
//             Finished row: thr = 0, nkeep = 0.
//
// How the kernel computes it.  One block of 1024 threads per row; the row is read once and held in registers as the
// order-preserving integer image of the float (key: sign bit flipped for positives, all bits for negatives), NPT keys
// per thread, wave w owning the contiguous span [w * 64 NPT, (w + 1) * 64 NPT) and lane l its elements j * 64 + l.
// Weights are 64-bit fixed point, floor(exp2((l_i - m) log2(e) / T) * 2^40): a row's sum stays below 2^57, and integer
// sums are exact in any order, so LDS atomics and scans give the same bits on every run and for every batch size.
// A weight below 2^-40 of the maximum's counts as 0 (at most 2^-24 of W in total).
//   t_k   radix select over the key, 8 bits a pass from the top (2 passes for bf16 logits, 4 for fp32), on LDS count
//         histograms; t_p the same select on histograms of the fixed-point weights with target ceil(p W_k), the
//         product formed in fp64 (W_k can exceed 2^53, so the target is within 2^-52 W_k of the exact ceiling).
//         A histogram is kept in 16 copies (by lane & 15, 257 apart): logits crowd into a few exponent bins.
//   draw  q = floor(n W / 2^24) with u = n 2^-24; the token is the first index whose inclusive weight sum reaches
//         q + 1 (sum > u W for integer sums): the wave from the 16 wave totals, then that wave alone transposes its
//         weights through LDS so that each lane sums NPT consecutive elements, scans the lanes, and the lane that
//         crosses walks its run.  q + 1 <= W, so the fallback never triggers.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage): profiles/sample_decode.txt; no instantiation uses scratch.
#include "common.h"
#include "dropout_rng.h"

namespace {
constexpr int SNT = 1024, SNW = SNT / 64;
constexpr int COPIES = 16, CSTRIDE = 257;
constexpr uint32_t KEY_NINF = 0x007fffffu;      // key of -inf: the smallest key of a real element; 0 marks "no element"
constexpr int FIX = 40;

typedef unsigned long long u64;

// After each iteration of an unrolled sum over a thread's keys: the running sum is made opaque, or the optimiser turns
// the chain into a tree with every 64-bit weight live at once and the NPT = 52 / 64 instantiations spill.
#define PIN(x) asm volatile("" : "+v"(x))

__device__ __forceinline__ uint32_t key_of(float f) {
    if (f != f) f = -INFINITY;
    if (f == 0.f) f = 0.f;
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float val_of(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_up_u64(u64 v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_u64(v, m);
    return v;
}
// inclusive prefix sum over the lanes of a wave
__device__ __forceinline__ u64 wave_scan_u64(u64 v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 t = shfl_up_u64(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

struct Shared {
    u64 hist[COPIES * CSTRIDE + 64];    // count or weight histograms, 16 copies; later 64 runs of NPT + 1 weights
    u64 bins[256];                  // the copies summed, in descending digit order: bins[r] is digit 255 - r
    u64 red[SNW];
    u64 sel[2];                     // the select's answer: r, and the sum of the bins before r
};

__device__ __forceinline__ u64 block_sum_u64(u64 v, Shared& sh) {
    v = wave_sum_u64(v);
    if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 t = 0;
#pragma unroll 2
    for (int i = 0; i < SNW; ++i) t += sh.red[i];
    __syncthreads();
    return t;
}
__device__ __forceinline__ uint32_t block_max_u32(uint32_t v, Shared& sh) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, (uint32_t)__shfl_xor(v, m));
    if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll 2
    for (int i = 0; i < SNW; ++i) t = max(t, (uint32_t)sh.red[i]);
    __syncthreads();
    return t;
}

// After every thread has added into sh.hist: the largest digit d whose bins from the top sum to >= target.  Returns d,
// subtracts the sum of the bins above d from target, and leaves sh.hist zero for the next pass.
__device__ __forceinline__ uint32_t select_digit(Shared& sh, u64& target) {
    const int t = threadIdx.x;
    __syncthreads();
    if (t < 256) {
        u64 s = 0;
#pragma unroll 4
        for (int c = 0; c < COPIES; ++c) {
            s += sh.hist[c * CSTRIDE + t];
            sh.hist[c * CSTRIDE + t] = 0;
        }
        sh.bins[255 - t] = s;
    }
    __syncthreads();
    if (t < 64) {
        u64 v[4], s = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = sh.bins[4 * t + i];
            s += v[i];
        }
        const u64 incl = wave_scan_u64(s, t);
        const u64 hit = __ballot(incl >= target);
        const int first = hit ? __ffsll((long long)hit) - 1 : 63;
        if (t == first) {
            u64 before = incl - s;
            int i = 0;
            while (i < 3 && before + v[i] < target) before += v[i++];
            sh.sel[0] = (u64)(4 * t + i);
            sh.sel[1] = before;
        }
    }
    __syncthreads();
    const uint32_t d = 255u - (uint32_t)sh.sel[0];
    target -= sh.sel[1];
    return d;
}

template <typename T, int NPT>
__global__ __launch_bounds__(SNT) void sample_kernel(const T* __restrict__ logits, long ld, int V, float temp, int topk,
                                                     float topp, const long long* __restrict__ state,
                                                     const float* __restrict__ u_over, long long* __restrict__ tok,
                                                     long long* __restrict__ history, long ldh, long col0,
                                                     uint8_t* __restrict__ finished, long long eos,
                                                     float* __restrict__ thr_out, int* __restrict__ nkeep_out) {
    constexpr int PASSES = std::is_same<T, float>::value ? 4 : 2;
    __shared__ Shared sh;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int base = wv * (64 * NPT) + lane;

    auto finish = [&](long long token, float thr, int nkeep) {      // thread 0 alone
        tok[b] = token;
        const long long step = state[1];
        if (history && step >= 0 && col0 + step < ldh) history[(long)b * ldh + col0 + step] = token;
        if (finished && eos >= 0 && token == eos) finished[b] = 1;
        if (thr_out) thr_out[b] = thr;
        if (nkeep_out) nkeep_out[b] = nkeep;
    };

    if (finished && eos >= 0 && finished[b]) {
        if (t == 0) finish(eos, 0.f, 0);
        return;
    }
    for (int i = t; i < COPIES * CSTRIDE; i += SNT) sh.hist[i] = 0;

    uint32_t key[NPT];
    const T* row = logits + (long)b * ld;
    uint32_t kmax = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int i = base + j * 64;
        key[j] = i < V ? key_of(Ld<T>::get(row, i)) : 0u;
        kmax = max(kmax, key[j]);
    }
    kmax = block_max_u32(kmax, sh);             // also orders the zeroing of sh.hist before its first use
    if (kmax <= KEY_NINF) {
        if (t == 0) finish(0, -INFINITY, 0);
        return;
    }
    const float m = val_of(kmax);

    if (temp == 0.f) {
        uint32_t first = 0xffffffffu;
#pragma unroll
        for (int j = NPT - 1; j >= 0; --j)
            if (key[j] == kmax) first = (uint32_t)(base + j * 64);
        first = ~block_max_u32(~first, sh);
        if (t == 0) finish((long long)first, m, 1);
        return;
    }

    // top-k: the key of the k-th largest element
    uint32_t kth = KEY_NINF;
    if (topk >= 1 && topk < V) {
        u64 target = (u64)topk;
        uint32_t prefix = 0;
#pragma unroll 1
        for (int pass = 0; pass < PASSES; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t above = pass ? 0xffffffffu << (shift + 8) : 0u;
            u64* h = sh.hist + (lane & (COPIES - 1)) * CSTRIDE;
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                uint32_t kj = key[j];
                PIN(kj);        // nothing derived from a key outlives its iteration (see opaque below)
                if (kj && (kj & above) == prefix) atomicAdd(h + ((kj >> shift) & 255u), (u64)1);
            }
            prefix |= select_digit(sh, target) << shift;
        }
        // bf16: a negative value's key has all sixteen low bits set, a positive one's none
        kth = PASSES == 2 && !(prefix & 0x80000000u) ? (prefix | 0xffffu) : prefix;
    }

    const float c = 1.44269504088896340736f / temp;
    auto weight_c = [&](uint32_t k, uint32_t floor_key, float mm, float cc) -> u64 {
        if (k < floor_key || k <= KEY_NINF) return 0;
        const float f = val_of(k);
        const float a = f == mm ? 0.f : (f - mm) * cc;
        if (!(a >= -(float)FIX)) return 0;
        return (u64)ldexpf(__builtin_amdgcn_exp2f(a), FIX);
    };
    // Every loop over the keys recomputes its weights from copies of m and c the optimiser cannot see through: a weight
    // shared between two loops (or between the passes of a select) is two more registers a key held across them, and
    // the NPT = 52 / 64 instantiations would spill.
    auto opaque = [](float x) {
        asm volatile("" : "+v"(x));
        return x;
    };

    // top-p: the largest key whose weights from the top reach ceil(p W_k)
    uint32_t thr_key = kth;
    if (topp > 0.f && topp < 1.f) {
        u64 s = 0;
        const float cs = opaque(c), ms = opaque(m);
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            s += weight_c(key[j], kth, ms, cs);
            PIN(s);
        }
        const u64 Wk = block_sum_u64(s, sh);
        u64 target = (u64)ceil((double)topp * (double)Wk);
        target = target < 1 ? 1 : (target > Wk ? Wk : target);
        uint32_t prefix = 0;
#pragma unroll 1
        for (int pass = 0; pass < PASSES; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t above = pass ? 0xffffffffu << (shift + 8) : 0u;
            u64* h = sh.hist + (lane & (COPIES - 1)) * CSTRIDE;
            const float cp = opaque(c), mp = opaque(m);
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                uint32_t kj = key[j];
                PIN(kj);
                if (kj >= kth && (kj & above) == prefix) {
                    const u64 w = weight_c(kj, kth, mp, cp);
                    if (w) atomicAdd(h + ((kj >> shift) & 255u), w);
                }
            }
            prefix |= select_digit(sh, target) << shift;
        }
        thr_key = PASSES == 2 && !(prefix & 0x80000000u) ? (prefix | 0xffffu) : prefix;
        if (thr_key < kth) thr_key = kth;
    }

    // the final set: count and weight
    u64 s = 0;
    uint32_t cnt = 0;
    const float cf = opaque(c), mf = opaque(m);
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        s += weight_c(key[j], thr_key, mf, cf);
        cnt += key[j] >= thr_key ? 1u : 0u;
        PIN(s);
    }
    const u64 nkeep = block_sum_u64((u64)cnt, sh);
    const u64 wave_w = wave_sum_u64(s);
    if (lane == 0) sh.red[wv] = wave_w;
    __syncthreads();
    u64 W = 0;
#pragma unroll 2
    for (int i = 0; i < SNW; ++i) W += sh.red[i];

    uint32_t n;
    if (u_over) {
        const float u = u_over[b];
        n = u >= 0.f ? (uint32_t)fminf(u * 16777216.f, 16777215.f) : 0u;     // NaN -> 0
    } else {
        const pdrop::Key kk = pdrop::stream_key(state, pdrop::SITE_SAMPLE, (uint32_t)b);
        n = pdrop::word(kk, 0) >> 8;
    }
    // need = floor(n W / 2^24) + 1, n < 2^24, W < 2^57: the first inclusive sum >= need is the first > u W
    const u64 need = ((__umul64hi((u64)n, W) << 40) | (((u64)n * W) >> 24)) + 1;
    u64 rem = 0, acc = 0;
    int target_wave = -1;
#pragma unroll 2
    for (int i = 0; i < SNW; ++i) {
        const u64 r = sh.red[i];
        if (target_wave < 0 && acc + r >= need) {
            target_wave = i;
            rem = need - acc;
        }
        acc += r;
    }
    // The wave that holds the crossing lays its weights out in LDS (the histogram's space, free by now) so that lane
    // l can walk the NPT consecutive elements l * NPT .. of the wave's span: run r starts at r * (NPT + 1), one word
    // of padding per run against bank conflicts.
    u64* wl = sh.hist;
    if (wv == target_wave) {
        const float cw = opaque(c), mw = opaque(m);
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int e = j * 64 + lane;
            wl[e + e / NPT] = weight_c(key[j], thr_key, mw, cw);
        }
    }
    __syncthreads();
    if (wv != target_wave) return;
    const u64* run = wl + lane * (NPT + 1);
    u64 mine = 0;
#pragma unroll 4
    for (int i = 0; i < NPT; ++i) mine += run[i];
    const u64 incl = wave_scan_u64(mine, lane);
    const u64 hit = __ballot(incl >= rem);
    if (lane != (hit ? __ffsll((long long)hit) - 1 : 63)) return;
    rem -= incl - mine;
    int i = 0;
#pragma unroll 1
    for (u64 a = 0; i < NPT - 1; ++i) {
        a += run[i];
        if (a >= rem) break;
    }
    finish((long long)(wv * (64 * NPT) + lane * NPT + i), val_of(thr_key), (int)nkeep);
}

template <typename T, int NPT>
void launch(const void* logits, long ld, int B, int V, float temp, int k, float p, const long long* state,
            const float* u_over, long long* tok, long long* history, long ldh, long col0, uint8_t* finished,
            long long eos, float* thr, int* nkeep, hipStream_t st) {
    hipLaunchKernelGGL((sample_kernel<T, NPT>), dim3(B), dim3(SNT), 0, st, (const T*)logits, ld, V, temp, k, p, state,
                       u_over, tok, history, ldh, col0, finished, eos, thr, nkeep);
}
}  // namespace

// logits [B] rows of V values ld apart, dtype 0 bf16 / 1 fp32; k = 0 and p = 0 mean no filter; eos < 0 means none.
// state int64[2]; u_over fp32 [B] or null; tok int64 [B]; history int64 [B][ldh] or null, written at column
// col0 + state.step when that is inside the row; finished uint8 [B] or null; thr fp32 [B], nkeep int32 [B] or null.
PDNN_API int pdnn_sample_logits(const void* logits, int dtype, long ld, int B, int V, float temp, int k, float p,
                                const long long* state, const float* u_over, long long* tok, long long* history,
                                long ldh, long col0, uint8_t* finished, long eos, float* thr, int* nkeep,
                                hipStream_t st) {
    if (!logits || !state || !tok || (dtype != 0 && dtype != 1) || B < 1 || V < 1 || V > 65536 || ld < V ||
        !(temp >= 0.f) || k < 0 || !(p >= 0.f) || (history && (ldh < 1 || col0 < 0 || col0 >= ldh)))
        return (int)hipErrorInvalidValue;
    if (p >= 1.f) p = 0.f;
    if (k >= V) k = 0;
#define PDNN_SAMPLE_GO(NPT)                                                                                           \
    do {                                                                                                              \
        if (dtype == 0)                                                                                               \
            launch<bf16_t, NPT>(logits, ld, B, V, temp, k, p, state, u_over, tok, history, ldh, col0, finished, eos,  \
                                thr, nkeep, st);                                                                      \
        else                                                                                                          \
            launch<float, NPT>(logits, ld, B, V, temp, k, p, state, u_over, tok, history, ldh, col0, finished, eos,   \
                               thr, nkeep, st);                                                                       \
    } while (0)
    if (V <= 4 * SNT) PDNN_SAMPLE_GO(4);
    else if (V <= 16 * SNT) PDNN_SAMPLE_GO(16);
    else if (V <= 52 * SNT) PDNN_SAMPLE_GO(52);
    else PDNN_SAMPLE_GO(64);
#undef PDNN_SAMPLE_GO
    PDNN_LAUNCH_RET;
}
