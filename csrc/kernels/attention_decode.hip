// Single-query causal attention against a key/value cache (GPT-2 generation), head dim 64, bf16 operands, fp32
// softmax and accumulation: the decode half of attention.hip.
//
// Cache layout (per layer): kcache, vcache bf16 [B][H][Tmax][64], head-major, so the keys of one (b, h) are contiguous
// 128-byte rows.  lens int32 [B] on the device: the number of tokens of sequence b already in the cache.  It is read by
// the kernels and never by the host, so a captured step can be replayed while lens advances; the kernels do not change
// it.  p = lens[b] is clamped into [0, Tmax - 1] before it becomes an address (a malformed lens gives wrong numbers,
// never an out-of-range access: the rule of the DOC kernels of attention.hip).
//
// pdnn_attn_decode: qkv bf16 [B][3*H*64] is the packed c_attn output of the one new token per sequence (columns h*64 = q,
// D + h*64 = k, 2D + h*64 = v, as in attention.hip).  For every (b, h) the new k and v rows are stored into cache slot p
// and out[b][h*64 ..] = softmax over keys 0..p (the new key included) times V.
//
// Split over keys (flash-decoding): the grid is static at B*H*ceil(Tmax / CHUNK) blocks, one block = one chunk of CHUNK
// keys of one (b, h).  A block whose chunk lies wholly past p writes a neutral partial (m = -inf, l = 0, o = 0) and
// leaves.  Every other block computes the CHUNK scaled scores t = c * q.k (c = scale * log2 e) into LDS, their maximum m,
// P = exp2(t - m) kept in fp32 (P is NOT rounded to bf16 before the V product), l = sum P and o = P V, and writes
// (m, l, o[64]) in fp32 to the caller's scratch ``part``: o at part[blk][64], (m, l) at part[nblk*64 + 2*blk].  A second
// launch (attn_decode_combine_kernel, one block per (b, h)) rescales every partial by exp2(m_i - M), sums l and o in
// chunk order and writes bf16 out = o / l.  With one chunk the first kernel writes out directly.
//
// No race by construction: the block whose chunk holds slot p takes the new key and value from qkv (never from the
// cache) and is the only writer of that slot; every block reads only slots < p from the cache; slots > p are never read
// and may hold anything.  No atomics, every sum in a fixed order: results repeat bitwise.
//
// Thread layout of a block (256 threads): 8 lanes share one key (16 bytes = 8 dims each), so one pass covers 32 keys and
// a chunk takes CHUNK / 32 passes; all K and V rows of the chunk are loaded before the first use (the kernel is
// bandwidth-bound: 2 * 128 bytes per key for 128 FLOPs, fp32 FMAs, no MFMA).
//
// pdnn_attn_decode_multi: 1 <= S <= 8 new tokens per sequence in one call (the verify step of speculative decoding).
// qkv bf16 [B*S][3*H*64], out bf16 [B*S][H*64]; row r = b*S + j is the query at position p_j = lens[b] + j and sees the
// cache keys 0 .. lens[b]-1 and the new keys of rows b*S .. b*S+j, which come from qkv and never from the cache.  All S new
// K and V rows go into slots lens[b] .. lens[b]+S-1 (a slot >= Tmax is not stored); lens is not changed.  Same static
// grid: one block per (b, h, chunk) loads the chunk's K and V once into registers and serves the S queries from them, one
// after the other (phase 1: the S score rows and their maxima into LDS; phase 2, per query: P, l, o).  Every query's
// arithmetic is the single-query kernel's (score8 / chunk_tail below are shared, the chunk boundaries are absolute), so
// out[b*S + j] and the cache slots equal, bit for bit, S successive pdnn_attn_decode calls with lens advanced by one
// between them.  Partials are indexed by (row r, h, chunk), so the combine kernel runs unchanged over B*S*H blocks; a
// chunk wholly past p_j writes that query's neutral partial.  No race: cache reads are of slots < lens[b] only, cache
// writes of slots >= lens[b] only, each by the one block whose chunk holds the slot.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), multi kernel, CHUNK 64 / 128 / 256:
//   VGPRs 48 / 74 / 129, LDS 10368 / 12416 / 16512 bytes, scratch 0 in every instantiation.
//
// pdnn_kv_cache_fill: prefill, the transposing copy of the K and V columns of qkv [B*T][3*H*64] into slots 0..T-1.
#include "common.h"

namespace {
constexpr int HD = 64;              // head dim
constexpr int NTD = 256;            // threads per block
constexpr int KPP = NTD / 8;        // keys per pass
constexpr int MAXS = 8;             // most queries per sequence of the multi-query kernel
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ int clamp_len(int p, int Tmax) { return min(max(p, 0), Tmax - 1); }

// sum over the 8 lanes that share a key (DPP: quad, quad pair, half row); every lane of the 8 gets the total
__device__ __forceinline__ float sum8(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    return v;
}

// scaled score of one key for the 8 lanes that share it: q.k in fp32, dims in order, then the 8-lane sum, times c
__device__ __forceinline__ float score8(const float* q, const u16x8_t& krow, float c) {
    float kf[8], s = 0.f;
    unpack8(krow, kf);
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(q[e], kf[e], s);
    return sum8(s) * c;
}

// the last step of a chunk, by the threads tid < HD (one wave): l = sum of the chunk's P in ascending key order (every
// lane, same order), o[tid] = sum over the KPP key slots in order; written as the final bf16 row (one chunk) or the partial
template <int CHUNK>
__device__ __forceinline__ void chunk_tail(const float* sc, const float (*red)[HD], int tid, float m, bool direct,
                                           bf16_t* orow, float* po, float* pml) {
    float l = 0.f;
#pragma unroll 8
    for (int j = 0; j < CHUNK; ++j) l += sc[j];
    float o = 0.f;
#pragma unroll
    for (int j = 0; j < KPP; ++j) o += red[j][tid];
    if (direct) {
        orow[tid] = f2bf(o / l);
    } else {
        po[tid] = o;
        if (tid == 0) {
            pml[0] = m;
            pml[1] = l;
        }
    }
}

template <int CHUNK>
__global__ void __launch_bounds__(NTD) attn_decode_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kcache,
                                                          bf16_t* __restrict__ vcache, const int* __restrict__ lens,
                                                          bf16_t* __restrict__ out, float* __restrict__ part, int H,
                                                          int Tmax, int nchunk, float scale) {
    constexpr int NP = CHUNK / KPP;                         // passes
    __shared__ float sc[CHUNK];                             // scaled scores, then P
    __shared__ __attribute__((aligned(16))) float red[KPP][HD];
    __shared__ float wred[NTD / 64];
    const int tid = threadIdx.x, slot = tid >> 3, sub = tid & 7;
    const int blk = blockIdx.x, ch = blk % nchunk, bh = blk / nchunk, h = bh % H, b = bh / H;
    const int p = clamp_len(lens[b], Tmax);
    const int k0 = ch * CHUNK;
    const int D = H * HD;
    float* po = part + (long)blk * HD;
    float* pml = part + (long)gridDim.x * HD + 2L * blk;
    if (k0 > p) {                                           // block-uniform: nothing visible in this chunk
        if (tid < HD) po[tid] = 0.f;
        if (tid == 0) {
            pml[0] = -INFINITY;
            pml[1] = 0.f;
        }
        return;
    }
    const bf16_t* qrow = qkv + (long)b * 3 * D + h * HD + sub * 8;
    bf16_t* Kc = kcache + (long)bh * Tmax * HD + sub * 8;
    bf16_t* Vc = vcache + (long)bh * Tmax * HD + sub * 8;
    const u16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
    u16x8_t kr[NP], vr[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int key = k0 + i * KPP + slot;
        kr[i] = zero;
        vr[i] = zero;
        if (key < p) {
            kr[i] = *reinterpret_cast<const u16x8_t*>(Kc + (long)key * HD);
            vr[i] = *reinterpret_cast<const u16x8_t*>(Vc + (long)key * HD);
        } else if (key == p) {                              // the new token: from qkv, and into its cache slot
            kr[i] = *reinterpret_cast<const u16x8_t*>(qrow + D);
            vr[i] = *reinterpret_cast<const u16x8_t*>(qrow + 2 * D);
            *reinterpret_cast<u16x8_t*>(Kc + (long)key * HD) = kr[i];
            *reinterpret_cast<u16x8_t*>(Vc + (long)key * HD) = vr[i];
        }
    }
    float q[8];
    unpack8(*reinterpret_cast<const u16x8_t*>(qrow), q);
    const float c = scale * LOG2E;
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int key = k0 + i * KPP + slot;
        float s = score8(q, kr[i], c);
        if (key > p) s = -INFINITY;
        if (sub == 0) sc[i * KPP + slot] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) wred[tid >> 6] = mx;
    __syncthreads();
    const float m = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));      // finite: key k0 <= p is visible
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const float pk = __builtin_amdgcn_exp2f(sc[i * KPP + slot] - m);          // exp2(-inf) = 0 past p
        if (sub == 0) sc[i * KPP + slot] = pk;              // read above by these 8 lanes only, all of one wave
        float vf[8];
        unpack8(vr[i], vf);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(pk, vf[e], acc[e]);
    }
    *reinterpret_cast<f32x4_t*>(&red[slot][sub * 8]) = f32x4_t{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4_t*>(&red[slot][sub * 8 + 4]) = f32x4_t{acc[4], acc[5], acc[6], acc[7]};
    __syncthreads();
    if (tid < HD) chunk_tail<CHUNK>(sc, red, tid, m, nchunk == 1, out + (long)b * D + h * HD, po, pml);
}

// S queries per sequence: see the header.  Partial of (row r = b*S + j, h, chunk ch) at index (r*H + h)*nchunk + ch.
template <int CHUNK>
__global__ void __launch_bounds__(NTD) attn_decode_multi_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kcache,
                                                                bf16_t* __restrict__ vcache, const int* __restrict__ lens,
                                                                bf16_t* __restrict__ out, float* __restrict__ part, int S,
                                                                int H, int Tmax, int nchunk, float scale) {
    constexpr int NP = CHUNK / KPP;
    __shared__ float sc[MAXS][CHUNK];                       // per query: scaled scores, then P
    __shared__ __attribute__((aligned(16))) float red[KPP][HD];
    __shared__ float wred[MAXS][NTD / 64];
    const int tid = threadIdx.x, slot = tid >> 3, sub = tid & 7;
    const int blk = blockIdx.x, ch = blk % nchunk, bh = blk / nchunk, h = bh % H, b = bh / H;
    const int p0 = clamp_len(lens[b], Tmax);                // query j sits at p0 + j
    const int k0 = ch * CHUNK;
    const int D = H * HD;
    const long npart = (long)gridDim.x * S;
    const bf16_t* qrow0 = qkv + (long)b * S * 3 * D + h * HD + sub * 8;
    bf16_t* Kc = kcache + (long)bh * Tmax * HD + sub * 8;
    bf16_t* Vc = vcache + (long)bh * Tmax * HD + sub * 8;
    const u16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
    u16x8_t kr[NP], vr[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int key = k0 + i * KPP + slot;
        kr[i] = zero;
        vr[i] = zero;
        if (key < p0) {
            kr[i] = *reinterpret_cast<const u16x8_t*>(Kc + (long)key * HD);
            vr[i] = *reinterpret_cast<const u16x8_t*>(Vc + (long)key * HD);
        } else if (key - p0 < S) {                          // new token key - p0: from qkv, and into its cache slot
            const bf16_t* r = qrow0 + (long)(key - p0) * 3 * D;
            kr[i] = *reinterpret_cast<const u16x8_t*>(r + D);
            vr[i] = *reinterpret_cast<const u16x8_t*>(r + 2 * D);
            if (key < Tmax) {
                *reinterpret_cast<u16x8_t*>(Kc + (long)key * HD) = kr[i];
                *reinterpret_cast<u16x8_t*>(Vc + (long)key * HD) = vr[i];
            }
        }
    }
    const float c = scale * LOG2E;
    for (int j = 0; j < S; ++j) {                           // phase 1; every branch on j is block-uniform
        const int p = p0 + j;
        if (k0 > p) continue;
        float q[8];
        unpack8(*reinterpret_cast<const u16x8_t*>(qrow0 + (long)j * 3 * D), q);
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int key = k0 + i * KPP + slot;
            float s = score8(q, kr[i], c);
            if (key > p) s = -INFINITY;
            if (sub == 0) sc[j][i * KPP + slot] = s;
            mx = fmaxf(mx, s);
        }
        mx = wave_max(mx);
        if ((tid & 63) == 0) wred[j][tid >> 6] = mx;
    }
    __syncthreads();
    for (int j = 0; j < S; ++j) {                           // phase 2
        const int p = p0 + j;
        const long pb = ((long)(b * S + j) * H + h) * nchunk + ch;
        float* po = part + pb * HD;
        float* pml = part + npart * HD + 2 * pb;
        if (k0 > p) {                                       // nothing visible to this query in this chunk
            if (tid < HD) po[tid] = 0.f;
            if (tid == 0) {
                pml[0] = -INFINITY;
                pml[1] = 0.f;
            }
            continue;
        }
        const float m = fmaxf(fmaxf(wred[j][0], wred[j][1]), fmaxf(wred[j][2], wred[j][3]));
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const float pk = __builtin_amdgcn_exp2f(sc[j][i * KPP + slot] - m);
            if (sub == 0) sc[j][i * KPP + slot] = pk;
            float vf[8];
            unpack8(vr[i], vf);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(pk, vf[e], acc[e]);
        }
        *reinterpret_cast<f32x4_t*>(&red[slot][sub * 8]) = f32x4_t{acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<f32x4_t*>(&red[slot][sub * 8 + 4]) = f32x4_t{acc[4], acc[5], acc[6], acc[7]};
        __syncthreads();
        if (tid < HD)
            chunk_tail<CHUNK>(sc[j], red, tid, m, nchunk == 1, out + (long)(b * S + j) * D + h * HD, po, pml);
        __syncthreads();                                    // red is reused by the next query
    }
}

// one block (64 threads = the 64 dims) per (b, h): out = sum_i w_i o_i / sum_i w_i l_i, w_i = exp2(m_i - M), chunk order
__global__ void __launch_bounds__(64) attn_decode_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ out,
                                                                 int nchunk) {
    const int bh = blockIdx.x, d = threadIdx.x;
    const long blk0 = (long)bh * nchunk;
    const float* po = part + blk0 * HD;
    const float* pml = part + (long)gridDim.x * nchunk * HD + 2 * blk0;
    float M = -INFINITY;
    for (int i = 0; i < nchunk; ++i) M = fmaxf(M, pml[2 * i]);      // chunk 0 is never neutral: M is finite
    float L = 0.f, O = 0.f;
    for (int i = 0; i < nchunk; ++i) {
        const float w = __builtin_amdgcn_exp2f(pml[2 * i] - M);     // neutral partial: exp2(-inf) = 0
        L = fmaf(w, pml[2 * i + 1], L);
        O = fmaf(w, po[(long)i * HD + d], O);
    }
    out[(long)bh * HD + d] = f2bf(O / L);
}

// 16-byte units: (b, h, t, sub) with sub fastest, so the cache is written in whole contiguous rows
__global__ void __launch_bounds__(NTD) kv_cache_fill_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kcache,
                                                            bf16_t* __restrict__ vcache, int T, int H, int Tmax,
                                                            long total) {
    const int D = H * HD;
    for (long i = (long)blockIdx.x * NTD + threadIdx.x; i < total; i += (long)gridDim.x * NTD) {
        const int sub = (int)(i & 7);
        const long r = i >> 3;
        const int t = (int)(r % T);
        const long bh = r / T;
        const int h = (int)(bh % H);
        const long b = bh / H;
        const bf16_t* src = qkv + (b * T + t) * 3L * D + h * HD + sub * 8;
        const long dst = (bh * Tmax + t) * HD + sub * 8;
        *reinterpret_cast<u16x8_t*>(kcache + dst) = *reinterpret_cast<const u16x8_t*>(src + D);
        *reinterpret_cast<u16x8_t*>(vcache + dst) = *reinterpret_cast<const u16x8_t*>(src + 2 * D);
    }
}

template <int CHUNK>
void launch_decode(const bf16_t* qkv, bf16_t* kcache, bf16_t* vcache, const int* lens, bf16_t* out, float* part, int B,
                   int H, int Tmax, float scale, hipStream_t st) {
    const int nchunk = (int)cdiv(Tmax, CHUNK);
    hipLaunchKernelGGL((attn_decode_kernel<CHUNK>), dim3(B * H * nchunk), dim3(NTD), 0, st, qkv, kcache, vcache, lens,
                       out, part, H, Tmax, nchunk, scale);
    if (nchunk > 1)
        hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(B * H), dim3(64), 0, st, (const float*)part, out, nchunk);
}

template <int CHUNK>
void launch_decode_multi(const bf16_t* qkv, bf16_t* kcache, bf16_t* vcache, const int* lens, bf16_t* out, float* part,
                         int B, int S, int H, int Tmax, float scale, hipStream_t st) {
    const int nchunk = (int)cdiv(Tmax, CHUNK);
    hipLaunchKernelGGL((attn_decode_multi_kernel<CHUNK>), dim3(B * H * nchunk), dim3(NTD), 0, st, qkv, kcache, vcache,
                       lens, out, part, S, H, Tmax, nchunk, scale);
    if (nchunk > 1)
        hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(B * S * H), dim3(64), 0, st, (const float*)part, out, nchunk);
}
}  // namespace

// fp32 elements of the scratch ``part`` that pdnn_attn_decode needs (0 on bad arguments)
PDNN_API int pdnn_attn_decode_ws(int B, int H, int Tmax, int chunk) {
    if (B < 1 || H < 1 || Tmax < 1 || (chunk != 64 && chunk != 128 && chunk != 256)) return 0;
    const long n = (long)B * H * cdiv(Tmax, chunk) * (HD + 2);
    return n > 0x7fffffffL ? 0 : (int)n;
}

// qkv [B][3*H*64] bf16, kcache / vcache [B][H][Tmax][64] bf16, lens int32 [B] (device), out [B][H*64] bf16,
// part fp32 [pdnn_attn_decode_ws].  chunk in {64, 128, 256}.
PDNN_API int pdnn_attn_decode(const bf16_t* qkv, bf16_t* kcache, bf16_t* vcache, const int* lens, bf16_t* out,
                              float* part, int B, int H, int Tmax, int chunk, float scale, hipStream_t st) {
    if (B < 1 || H < 1 || Tmax < 1 || !qkv || !kcache || !vcache || !lens || !out || !part)
        return (int)hipErrorInvalidValue;
    if (pdnn_attn_decode_ws(B, H, Tmax, chunk) == 0) return (int)hipErrorInvalidValue;
    if (chunk == 64)
        launch_decode<64>(qkv, kcache, vcache, lens, out, part, B, H, Tmax, scale, st);
    else if (chunk == 128)
        launch_decode<128>(qkv, kcache, vcache, lens, out, part, B, H, Tmax, scale, st);
    else
        launch_decode<256>(qkv, kcache, vcache, lens, out, part, B, H, Tmax, scale, st);
    PDNN_LAUNCH_RET;
}

// prefill: qkv [B*T][3*H*64] bf16, T <= Tmax: K and V of every (b, t, h) into slot t; slots >= T are untouched
PDNN_API int pdnn_kv_cache_fill(const bf16_t* qkv, bf16_t* kcache, bf16_t* vcache, int B, int T, int H, int Tmax,
                                hipStream_t st) {
    if (B < 1 || T < 1 || H < 1 || Tmax < 1 || T > Tmax || !qkv || !kcache || !vcache) return (int)hipErrorInvalidValue;
    const long total = (long)B * H * T * 8;
    hipLaunchKernelGGL(kv_cache_fill_kernel, dim3(stream_grid(total, NTD)), dim3(NTD), 0, st, qkv, kcache, vcache, T, H,
                       Tmax, total);
    PDNN_LAUNCH_RET;
}

// fp32 elements of the scratch ``part`` that pdnn_attn_decode_multi needs (0 on bad arguments)
PDNN_API int pdnn_attn_decode_multi_ws(int B, int S, int H, int Tmax, int chunk) {
    if (B < 1 || S < 1 || S > MAXS) return 0;
    const long rows = (long)B * S;
    return rows > 0x7fffffffL ? 0 : pdnn_attn_decode_ws((int)rows, H, Tmax, chunk);
}

// qkv [B*S][3*H*64] bf16, kcache / vcache [B][H][Tmax][64] bf16, lens int32 [B] (device), out [B*S][H*64] bf16,
// part fp32 [pdnn_attn_decode_multi_ws].  1 <= S <= 8, chunk in {64, 128, 256}.
PDNN_API int pdnn_attn_decode_multi(const bf16_t* qkv, bf16_t* kcache, bf16_t* vcache, const int* lens, bf16_t* out,
                                    float* part, int B, int S, int H, int Tmax, int chunk, float scale, hipStream_t st) {
    if (B < 1 || H < 1 || Tmax < 1 || !qkv || !kcache || !vcache || !lens || !out || !part)
        return (int)hipErrorInvalidValue;
    if (pdnn_attn_decode_multi_ws(B, S, H, Tmax, chunk) == 0) return (int)hipErrorInvalidValue;
    if (chunk == 64)
        launch_decode_multi<64>(qkv, kcache, vcache, lens, out, part, B, S, H, Tmax, scale, st);
    else if (chunk == 128)
        launch_decode_multi<128>(qkv, kcache, vcache, lens, out, part, B, S, H, Tmax, scale, st);
    else
        launch_decode_multi<256>(qkv, kcache, vcache, lens, out, part, B, S, H, Tmax, scale, st);
    PDNN_LAUNCH_RET;
}
