// Single-query and multi-query causal attention against a key/value cache at head dim 128 (GPT-2 generation), bf16
// operands, fp32 softmax and accumulation: the head-dim-128 set of attention_decode.hip's three entries, with kernels of
// its own (that file is untouched and its kernels keep their bits).
//
// Contract: that of attention_decode.hip's header with 128 in place of 64.  Cache (per layer): kcache, vcache bf16
// [B][H][Tmax][128], head-major, 256-byte rows.  lens int32 [B] on the device, read by the kernels only and never changed;
// p = lens[b] is clamped into [0, Tmax - 1] before it becomes an address (a malformed lens gives wrong numbers, never an
// out-of-range access).
//
// pdnn_attn_decode_hd128: qkv bf16 [B][3*H*128] (columns h*128 = q, D + h*128 = k, 2D + h*128 = v).  For every (b, h)
// the new k and v rows go into cache slot p and out[b][h*128 ..] = softmax over keys 0..p (the new key included) times V.
// Split over keys: a static grid of B*H*ceil(Tmax / CHUNK) blocks, one block = one chunk of CHUNK keys of one (b, h).  A
// block whose chunk lies wholly past p writes a neutral partial (m = -inf, l = 0, o = 0).  Every other block computes the
// scaled scores t = c * q.k (c = scale * log2 e), their maximum m, P = exp2(t - m) in fp32 (never rounded to bf16), l =
// sum P, o = P V, and writes (m, l, o[128]) in fp32 to the caller's ``part``: o at part[blk][128], (m, l) at
// part[nblk*128 + 2*blk].  A second launch (one block of 128 threads per (b, h)) rescales every partial by exp2(m_i - M),
// sums l and o in chunk order and writes bf16 out = o / l.  With one chunk the first kernel writes out directly.
//
// No race by construction: the block whose chunk holds slot p takes the new key and value from qkv (never from the cache)
// and is the only writer of that slot; cache reads are of slots < p only; slots > p are never read and may hold anything.
// No atomics, every sum in a fixed order: results repeat bitwise.
//
// Design.  A 256-byte row is shared by 16 lanes at 16 bytes (8 dims) each, one DPP row, so the per-key dot product is 8
// FMAs and the four DPP steps of row16_sum, after which all 16 lanes hold the same bits.  A block has 256 threads (16 keys
// per pass) at CHUNK 64 and 128 and 512 threads (32 keys per pass) at CHUNK 256, so a lane never holds more than 8 K and
// 8 V rows (64 VGPRs): the doubled row is paid with threads, not registers, and the multi-query kernel has room for its
// queries.  All K and V loads of the chunk are issued before the first use (bandwidth-bound: 512 bytes per key for 256
// FLOPs, fp32 FMAs, no MFMA).  The scores stay in registers (the 16 lanes of a key all hold them), so the single-query
// kernel keeps no score array in LDS: one barrier for the block maximum, one for the cross-key reduction.  l is summed per
// key slot over the passes, then over the slots in order by the tail, next to o: CHUNK/16 + 16 additions, not CHUNK.
//
// pdnn_attn_decode_multi_hd128: 1 <= S <= 8 new tokens per sequence in one call.  qkv bf16 [B*S][3*H*128], out bf16
// [B*S][H*128]; row r = b*S + j is the query at position p_j = lens[b] + j and sees the cache keys 0 .. lens[b]-1 and the
// new keys of rows b*S .. b*S+j, which come from qkv and never from the cache.  The S new K and V rows go into slots
// lens[b] .. lens[b]+S-1; a slot >= Tmax is not stored.  Same static grid: one block per (b, h, chunk) loads the chunk's K
// and V once and serves the S queries from those registers (phase 1: the S score rows into LDS and the per-wave maxima;
// phase 2, per query: P, l, o through a double-buffered reduction array, one barrier per query).  Every query runs
// chunk_scores / chunk_pv / chunk_tail, the single-query kernel's own device functions, on absolute chunk boundaries, so
// out[b*S + j] and the cache equal, bit for bit, S successive pdnn_attn_decode_hd128 calls with lens advanced by one
// between them.  That holds past the end of the cache too: a single-query call at lens >= Tmax lands on slot Tmax - 1
// (the clamp), sees slots 0 .. Tmax-2 and its own key, and leaves its k, v there.  So a query with p_j > Tmax - 1 scores
// slot Tmax - 1 from its own row (the OV instantiations, taken by a block-uniform branch), and slot Tmax - 1 ends as the
// last row that reaches it.  Partials are indexed by (row r, h, chunk), so the combine runs unchanged over B*S*H blocks.
//
// pdnn_kv_cache_fill_hd128: prefill, the transposing copy of the K and V columns of qkv [B*T][3*H*128] into slots 0..T-1,
// 16 bytes per access on both sides; slots >= T are untouched.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, built without packed fp32 ops), CHUNK 64 / 128 / 256:
//   single: VGPRs 58 / 93 / 98, LDS 8272 / 8272 / 16544 bytes, scratch 0
//   multi:  VGPRs 100 / 167 / 167, LDS 18688 / 20736 / 41472 bytes, scratch 0 (512 threads leave 256 VGPRs per lane)
//   combine: VGPRs 8, fill: VGPRs 26, no LDS, scratch 0
#include "common.h"

namespace {
constexpr int HD = 128;             // head dim
constexpr int LPK = 16;             // lanes per key: 16 bytes of the 256-byte row each
constexpr int MAXS = 8;             // most queries per sequence of the multi-query kernel
constexpr float LOG2E = 1.4426950408889634f;

constexpr int nthreads(int chunk) { return chunk == 256 ? 512 : 256; }

__device__ __forceinline__ int clamp_len(int p, int Tmax) { return min(max(p, 0), Tmax - 1); }
__device__ __forceinline__ u16x8_t ld8(const bf16_t* p) { return *reinterpret_cast<const u16x8_t*>(p); }
__device__ __forceinline__ void st8(bf16_t* p, const u16x8_t& v) { *reinterpret_cast<u16x8_t*>(p) = v; }

// Scaled scores of this lane's NP keys key0 + i*KPP, -inf past p, into s (the 16 lanes of a key get the same bits);
// returns their maximum.  OV (multi-query kernel, a query past the end of the cache): key ovkey is scored from kov.
template <int NP, int KPP, bool OV>
__device__ __forceinline__ float chunk_scores(const float* q, const u16x8_t* kr, const u16x8_t& kov, int ovkey, int key0,
                                              int p, float c, float* s) {
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int key = key0 + i * KPP;
        float kf[8], d = 0.f;
        unpack8(OV && key == ovkey ? kov : kr[i], kf);
#pragma unroll
        for (int e = 0; e < 8; ++e) d = fmaf(q[e], kf[e], d);
        s[i] = key > p ? -INFINITY : row16_sum(d) * c;
        mx = fmaxf(mx, s[i]);
    }
    return mx;
}

// P = exp2(s - m) of this lane's NP keys in pass order: l = sum P, acc[8] = sum P v over this lane's 8 dims
template <int NP, int KPP, bool OV>
__device__ __forceinline__ void chunk_pv(const float* s, float m, const u16x8_t* vr, const u16x8_t& vov, int ovkey,
                                         int key0, float* acc, float& l) {
    l = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const float pk = __builtin_amdgcn_exp2f(s[i] - m);          // exp2(-inf) = 0 past p
        l += pk;
        float vf[8];
        unpack8(OV && key0 + i * KPP == ovkey ? vov : vr[i], vf);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(pk, vf[e], acc[e]);
    }
}

// this lane's share of the cross-key reduction into LDS: red[slot][dims], lred[slot]
__device__ __forceinline__ void put_partial(float (*red)[HD], float* lred, int slot, int sub, const float* acc, float l) {
    *reinterpret_cast<f32x4_t*>(&red[slot][sub * 8]) = f32x4_t{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4_t*>(&red[slot][sub * 8 + 4]) = f32x4_t{acc[4], acc[5], acc[6], acc[7]};
    if (sub == 0) lred[slot] = l;
}

// the last step of a chunk, by the threads tid < HD: l and o[tid] summed over the KPP key slots in order (every lane the
// same l); written as the final bf16 row (one chunk) or as the partial
template <int KPP>
__device__ __forceinline__ void chunk_tail(const float (*red)[HD], const float* lred, int tid, float m, bool direct,
                                           bf16_t* orow, float* po, float* pml) {
    float l = 0.f, o = 0.f;
#pragma unroll
    for (int j = 0; j < KPP; ++j) {
        l += lred[j];
        o += red[j][tid];
    }
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

__device__ __forceinline__ void neutral_partial(int tid, float* po, float* pml) {
    if (tid < HD) po[tid] = 0.f;
    if (tid == 0) {
        pml[0] = -INFINITY;
        pml[1] = 0.f;
    }
}

template <int NW>
__device__ __forceinline__ float max_of(const float* w) {
    float m = w[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) m = fmaxf(m, w[i]);
    return m;
}

template <int CHUNK>
__global__ void __launch_bounds__(nthreads(CHUNK))
attn_decode_hd128_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache,
                         const int* __restrict__ lens, bf16_t* __restrict__ out, float* __restrict__ part, int H, int Tmax,
                         int nchunk, float scale) {
    constexpr int NT = nthreads(CHUNK), KPP = NT / LPK, NP = CHUNK / KPP, NW = NT / 64;
    __shared__ __attribute__((aligned(16))) float red[KPP][HD];
    __shared__ float lred[KPP];
    __shared__ float wred[NW];
    const int tid = threadIdx.x, slot = tid >> 4, sub = tid & 15;
    const int blk = blockIdx.x, ch = blk % nchunk, bh = blk / nchunk, h = bh % H, b = bh / H;
    const int p = clamp_len(lens[b], Tmax);
    const int k0 = ch * CHUNK;
    const int D = H * HD;
    float* po = part + (long)blk * HD;
    float* pml = part + (long)gridDim.x * HD + 2L * blk;
    if (k0 > p) {                                           // block-uniform: nothing visible in this chunk
        neutral_partial(tid, po, pml);
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
            kr[i] = ld8(Kc + (long)key * HD);
            vr[i] = ld8(Vc + (long)key * HD);
        } else if (key == p) {                              // the new token: from qkv, and into its cache slot
            kr[i] = ld8(qrow + D);
            vr[i] = ld8(qrow + 2 * D);
            st8(Kc + (long)key * HD, kr[i]);
            st8(Vc + (long)key * HD, vr[i]);
        }
    }
    float q[8], s[NP], acc[8], l;
    unpack8(ld8(qrow), q);
    float mx = chunk_scores<NP, KPP, false>(q, kr, zero, 0, k0 + slot, p, scale * LOG2E, s);
    mx = wave_max(mx);
    if ((tid & 63) == 0) wred[tid >> 6] = mx;
    __syncthreads();
    const float m = max_of<NW>(wred);                       // finite: key k0 <= p is visible
    chunk_pv<NP, KPP, false>(s, m, vr, zero, 0, k0 + slot, acc, l);
    put_partial(red, lred, slot, sub, acc, l);
    __syncthreads();
    if (tid < HD) chunk_tail<KPP>(red, lred, tid, m, nchunk == 1, out + (long)b * D + h * HD, po, pml);
}

// S queries per sequence: see the header.  Partial of (row r = b*S + j, h, chunk ch) at index (r*H + h)*nchunk + ch.
template <int CHUNK>
__global__ void __launch_bounds__(nthreads(CHUNK))
attn_decode_multi_hd128_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache,
                               const int* __restrict__ lens, bf16_t* __restrict__ out, float* __restrict__ part, int S,
                               int H, int Tmax, int nchunk, float scale) {
    constexpr int NT = nthreads(CHUNK), KPP = NT / LPK, NP = CHUNK / KPP, NW = NT / 64;
    __shared__ float sc[MAXS][CHUNK];                       // per query: scaled scores
    __shared__ __attribute__((aligned(16))) float red[2][KPP][HD];      // by query parity: no barrier after the tail
    __shared__ float lred[2][KPP];
    __shared__ float wred[MAXS][NW];
    const int tid = threadIdx.x, slot = tid >> 4, sub = tid & 15;
    const int blk = blockIdx.x, ch = blk % nchunk, bh = blk / nchunk, h = bh % H, b = bh / H;
    const int last = Tmax - 1;
    const int p0 = clamp_len(lens[b], Tmax);                // query j sits at min(p0 + j, last)
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
            kr[i] = ld8(Kc + (long)key * HD);
            vr[i] = ld8(Vc + (long)key * HD);
        } else if (key - p0 < S && key <= last) {           // new token key - p0: from qkv, and into its cache slot
            const bf16_t* r = qrow0 + (long)(key - p0) * 3 * D;
            kr[i] = ld8(r + D);
            vr[i] = ld8(r + 2 * D);
            // every query past the end lands on the last slot too, so that slot ends as the last row's
            const bf16_t* w = key == last ? qrow0 + (long)(S - 1) * 3 * D : r;
            st8(Kc + (long)key * HD, ld8(w + D));
            st8(Vc + (long)key * HD, ld8(w + 2 * D));
        }
    }
    const float c = scale * LOG2E;
    for (int j = 0; j < S; ++j) {                           // phase 1; every branch on j is block-uniform
        const int p = min(p0 + j, last);
        if (k0 > p) continue;
        const bf16_t* qr = qrow0 + (long)j * 3 * D;
        float q[8], s[NP], mx;
        unpack8(ld8(qr), q);
        if (p0 + j > last)
            mx = chunk_scores<NP, KPP, true>(q, kr, ld8(qr + D), last, k0 + slot, p, c, s);
        else
            mx = chunk_scores<NP, KPP, false>(q, kr, zero, 0, k0 + slot, p, c, s);
        if (sub == 0) {
#pragma unroll
            for (int i = 0; i < NP; ++i) sc[j][i * KPP + slot] = s[i];
        }
        mx = wave_max(mx);
        if ((tid & 63) == 0) wred[j][tid >> 6] = mx;
    }
    __syncthreads();
    for (int j = 0; j < S; ++j) {                           // phase 2
        const int p = min(p0 + j, last);
        const long pb = ((long)(b * S + j) * H + h) * nchunk + ch;
        float* po = part + pb * HD;
        float* pml = part + npart * HD + 2 * pb;
        if (k0 > p) {                                       // nothing visible to this query in this chunk
            neutral_partial(tid, po, pml);
            continue;
        }
        const float m = max_of<NW>(wred[j]);
        float s[NP], acc[8], l;
#pragma unroll
        for (int i = 0; i < NP; ++i) s[i] = sc[j][i * KPP + slot];
        if (p0 + j > last)
            chunk_pv<NP, KPP, true>(s, m, vr, ld8(qrow0 + (long)j * 3 * D + 2 * D), last, k0 + slot, acc, l);
        else
            chunk_pv<NP, KPP, false>(s, m, vr, zero, 0, k0 + slot, acc, l);
        put_partial(red[j & 1], lred[j & 1], slot, sub, acc, l);
        __syncthreads();                                    // also orders query j-1's tail before query j+1's writes
        if (tid < HD)
            chunk_tail<KPP>(red[j & 1], lred[j & 1], tid, m, nchunk == 1, out + (long)(b * S + j) * D + h * HD, po, pml);
    }
}

// one block (128 threads = the 128 dims) per (row, h): out = sum_i w_i o_i / sum_i w_i l_i, w_i = exp2(m_i - M), chunk order
__global__ void __launch_bounds__(HD) attn_decode_combine_hd128_kernel(const float* __restrict__ part,
                                                                       bf16_t* __restrict__ out, int nchunk) {
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

// 16-byte units: (b, h, t, sub) with sub fastest, so the cache is written in whole contiguous 256-byte rows
__global__ void __launch_bounds__(256) kv_cache_fill_hd128_kernel(const bf16_t* __restrict__ qkv,
                                                                  bf16_t* __restrict__ kcache,
                                                                  bf16_t* __restrict__ vcache, int T, int H, int Tmax,
                                                                  long total) {
    const int D = H * HD;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int sub = (int)(i & (LPK - 1));
        const long r = i / LPK;
        const int t = (int)(r % T);
        const long bh = r / T;
        const int h = (int)(bh % H);
        const long b = bh / H;
        const bf16_t* src = qkv + (b * T + t) * 3L * D + h * HD + sub * 8;
        const long dst = (bh * Tmax + t) * HD + sub * 8;
        st8(kcache + dst, ld8(src + D));
        st8(vcache + dst, ld8(src + 2 * D));
    }
}

template <int CHUNK>
void launch_decode(const bf16_t* qkv, bf16_t* kcache, bf16_t* vcache, const int* lens, bf16_t* out, float* part, int B,
                   int S, int H, int Tmax, float scale, hipStream_t st) {
    const int nchunk = (int)cdiv(Tmax, CHUNK);
    const dim3 grid(B * H * nchunk), block(nthreads(CHUNK));
    if (S == 0)                                             // the single-query entry
        hipLaunchKernelGGL((attn_decode_hd128_kernel<CHUNK>), grid, block, 0, st, qkv, kcache, vcache, lens, out, part, H,
                           Tmax, nchunk, scale);
    else
        hipLaunchKernelGGL((attn_decode_multi_hd128_kernel<CHUNK>), grid, block, 0, st, qkv, kcache, vcache, lens, out,
                           part, S, H, Tmax, nchunk, scale);
    if (nchunk > 1)
        hipLaunchKernelGGL(attn_decode_combine_hd128_kernel, dim3(B * (S ? S : 1) * H), dim3(HD), 0, st, (const float*)part,
                           out, nchunk);
}

int decode(const bf16_t* qkv, bf16_t* kcache, bf16_t* vcache, const int* lens, bf16_t* out, float* part, int B, int S,
           int H, int Tmax, int chunk, float scale, hipStream_t st) {
    if (chunk == 64)
        launch_decode<64>(qkv, kcache, vcache, lens, out, part, B, S, H, Tmax, scale, st);
    else if (chunk == 128)
        launch_decode<128>(qkv, kcache, vcache, lens, out, part, B, S, H, Tmax, scale, st);
    else
        launch_decode<256>(qkv, kcache, vcache, lens, out, part, B, S, H, Tmax, scale, st);
    PDNN_LAUNCH_RET;
}
}  // namespace

// fp32 elements of the scratch ``part`` that pdnn_attn_decode_hd128 needs (0 on bad arguments)
PDNN_API int pdnn_attn_decode_hd128_ws(int B, int H, int Tmax, int chunk) {
    if (B < 1 || H < 1 || Tmax < 1 || (chunk != 64 && chunk != 128 && chunk != 256)) return 0;
    const long n = (long)B * H * cdiv(Tmax, chunk) * (HD + 2);
    return n > 0x7fffffffL ? 0 : (int)n;
}

// qkv [B][3*H*128] bf16, kcache / vcache [B][H][Tmax][128] bf16, lens int32 [B] (device), out [B][H*128] bf16,
// part fp32 [pdnn_attn_decode_hd128_ws].  chunk in {64, 128, 256}.
PDNN_API int pdnn_attn_decode_hd128(const bf16_t* qkv, bf16_t* kcache, bf16_t* vcache, const int* lens, bf16_t* out,
                                    float* part, int B, int H, int Tmax, int chunk, float scale, hipStream_t st) {
    if (B < 1 || H < 1 || Tmax < 1 || !qkv || !kcache || !vcache || !lens || !out || !part)
        return (int)hipErrorInvalidValue;
    if (pdnn_attn_decode_hd128_ws(B, H, Tmax, chunk) == 0) return (int)hipErrorInvalidValue;
    return decode(qkv, kcache, vcache, lens, out, part, B, 0, H, Tmax, chunk, scale, st);
}

// prefill: qkv [B*T][3*H*128] bf16, T <= Tmax: K and V of every (b, t, h) into slot t; slots >= T are untouched
PDNN_API int pdnn_kv_cache_fill_hd128(const bf16_t* qkv, bf16_t* kcache, bf16_t* vcache, int B, int T, int H, int Tmax,
                                      hipStream_t st) {
    if (B < 1 || T < 1 || H < 1 || Tmax < 1 || T > Tmax || !qkv || !kcache || !vcache) return (int)hipErrorInvalidValue;
    const long total = (long)B * H * T * LPK;
    hipLaunchKernelGGL(kv_cache_fill_hd128_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, st, qkv, kcache, vcache, T,
                       H, Tmax, total);
    PDNN_LAUNCH_RET;
}

// fp32 elements of the scratch ``part`` that pdnn_attn_decode_multi_hd128 needs (0 on bad arguments)
PDNN_API int pdnn_attn_decode_multi_hd128_ws(int B, int S, int H, int Tmax, int chunk) {
    if (B < 1 || S < 1 || S > MAXS) return 0;
    const long rows = (long)B * S;
    return rows > 0x7fffffffL ? 0 : pdnn_attn_decode_hd128_ws((int)rows, H, Tmax, chunk);
}

// qkv [B*S][3*H*128] bf16, kcache / vcache [B][H][Tmax][128] bf16, lens int32 [B] (device), out [B*S][H*128] bf16,
// part fp32 [pdnn_attn_decode_multi_hd128_ws].  1 <= S <= 8, chunk in {64, 128, 256}.
PDNN_API int pdnn_attn_decode_multi_hd128(const bf16_t* qkv, bf16_t* kcache, bf16_t* vcache, const int* lens, bf16_t* out,
                                          float* part, int B, int S, int H, int Tmax, int chunk, float scale,
                                          hipStream_t st) {
    if (B < 1 || H < 1 || Tmax < 1 || !qkv || !kcache || !vcache || !lens || !out || !part)
        return (int)hipErrorInvalidValue;
    if (pdnn_attn_decode_multi_hd128_ws(B, S, H, Tmax, chunk) == 0) return (int)hipErrorInvalidValue;
    return decode(qkv, kcache, vcache, lens, out, part, B, S, H, Tmax, chunk, scale, st);
}
