// Many-query causal attention at an offset against a key/value cache (GPT-2 generation: a second chat turn, a chunk of
// a long prompt), head dim 64, bf16 operands, fp32 softmax and accumulation, on v_mfma_f32_16x16x32_bf16: the prefill
// half that attention_decode.hip lacks.  Cache layout and lens are attention_decode.hip's: kcache, vcache bf16
// [B][H][Tmax][64], lens int32 [B] on the device, read by the kernels and never by the host, never written here, so a
// captured append + extend follows lens on replay.
//
// pdnn_kv_cache_append: qkv bf16 [B*Tq][3*H*64] (packed as in attention.hip).  K and V of row b*Tq + j go to slot
// lens[b] + j; a slot >= Tmax is not stored.  Whole contiguous 128-byte rows, as kv_cache_fill.
//
// pdnn_attn_extend: runs after the append on the same stream and reads EVERY key, the new ones included, from the cache
// (no key comes from qkv, so there is no race inside the kernel to reason about).  Query j of sequence b sits at
// position p = lens[b] + j and sees exactly the keys 0..p; out bf16 [B*Tq][H*64].
//
// The kernel is attention.hip's forward (S^T = K Q^T, online softmax per lane with the lazy rescale, P^T consumed from
// the accumulator registers as the B operand of O^T += V^T P^T, V^T read with ds_read_b64_tr_b16) with these changes:
//   * one block = one tile of TILE = 64 queries of one (b, h), 4 waves x 16 queries (one query fragment per wave: a
//     64-token turn is one tile per head, and B * H * Tq / 64 blocks is what fills the machine at small B).  The grid
//     is static; heavy (late) query tiles come first.
//   * K and V tiles of 64 keys are staged from the contiguous cache rows of (b, h), at absolute key tiles 0, 64, ...,
//     up to the tile of the block's last visible key min(lens[b] + q_last, Tmax - 1): the trip count comes from
//     lens[b] on the device.  No split over keys, no atomics, one summation order: results repeat bitwise.
//   * the causal diagonal is shifted by lens[b], which is not tile-aligned: a wave masks only tiles that reach past the
//     limit of its FIRST query (wave-uniform, as ``diag`` in attention.hip) and skips tiles wholly past the limit of
//     its last one.
//   * address safety: lens[b] is clamped into [0, Tmax] before it becomes an address or a trip count, a key row index
//     is clamped to Tmax - 1, and a key >= Tmax is masked.  A malformed lens gives wrong numbers, never an
//     out-of-range access.
//   * slots past the last visible key may hold any bit pattern (NaN, Inf): scores are masked by select (a NaN score of
//     a masked key is replaced, never propagated), and a V row past the block's last visible key is zeroed while it is
//     staged, so that P = 0 never meets Inf or NaN in the MFMA.  Rows between a query's own limit and the block's
//     limit are this call's new keys, which the append has written.
// Padding query rows (a turn shorter than Tq) produce values nobody reads; causality keeps them invisible to real rows.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   attn_extend_kernel       122 VGPRs (0 AGPRs), 32768 bytes LDS, scratch 0, 4 waves / SIMD
//   kv_cache_append_kernel    22 VGPRs, 0 bytes LDS, scratch 0
#include "common.h"

namespace {
constexpr int HD = 64;          // head dim
constexpr int TILE = 64;        // queries per block
constexpr int NTA = 256;
constexpr float RESC = 8.f;     // lazy-rescale threshold (log2 units), attention.hip's
constexpr float LOG2E = 1.4426950408889634f;

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// The fragment helpers below are attention.hip's (same tile image, same operand order), copied so that its compiled
// kernels cannot change with this file.
// [64][64] bf16 tile image, 128-byte rows, 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7)
__device__ __forceinline__ int toff(int row, int chunk) { return row * HD + ((chunk ^ ((row >> 1) & 7)) << 3); }

// K-major fragment: lane -> row (row0 + (lane & 15)), k = 32 ks + 8 (lane >> 4) .. +7
__device__ __forceinline__ bf16x8_t frag_rows(const bf16_t* img, int row0, int ks, int lane) {
    const int row = row0 + (lane & 15);
    return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(img + toff(row, ks * 4 + (lane >> 4))));
}

// Transposed fragment over tile rows [32 kk, 32 kk + 32) in the permuted order of an accumulator-sourced operand: lane
// (col = col0 + (lane & 15), group g) receives rows 32kk + 4g + 0..3 and 32kk + 16 + 4g + 0..3 of column col
__device__ __forceinline__ bf16x8_t frag_tr_perm(const bf16_t* img, int col0, int kk, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int col = col0 + 4 * p;
    const int r0 = 32 * kk + 4 * g + q;
    const bf16_t* p0 = img + toff(r0, col >> 3) + (col & 7);
    const bf16_t* p1 = img + toff(r0 + 16, col >> 3) + (col & 7);
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p1));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, v);
}

// two fp32 accumulator fragments (rows 4g + r of fragment a and b) -> one bf16 B operand (permuted k)
__device__ __forceinline__ bf16x8_t pack_acc(const f32x4_t& a, const f32x4_t& b) {
    s16x8 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        v[r] = (short)f2bf(a[r]);
        v[4 + r] = (short)f2bf(b[r]);
    }
    return __builtin_bit_cast(bf16x8_t, v);
}

__device__ __forceinline__ f32x4_t mfma(const bf16x8_t& a, const bf16x8_t& b, const f32x4_t& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// global fragment load: row-major [rows][ld] source, lane -> row (lane & 15), 8 k at 32 ks + 8 g
__device__ __forceinline__ bf16x8_t gfrag(const bf16_t* base, long ld, int ks, int lane) {
    const bf16_t* p = base + (long)(lane & 15) * ld + ks * 32 + 8 * (lane >> 4);
    return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(p));
}

// 64-key tile of the cache rows of one (b, h): 256 threads x 2 chunks.  Row index clamped to Tmax - 1; a row past
// ``keep`` is zeroed (V: the block's last visible key; K: never, keep = INT_MAX)
struct CacheTile {
    u16x8_t r[2];
    __device__ __forceinline__ void load(const bf16_t* rows, int k0, int Tmax, int keep, int tid) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int key = k0 + (tid >> 3) + 32 * i, ch = tid & 7;
            r[i] = *reinterpret_cast<const u16x8_t*>(rows + (long)min(key, Tmax - 1) * HD + ch * 8);
            if (key > keep) r[i] = u16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    __device__ __forceinline__ void store(bf16_t* img, int tid) const {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (tid >> 3) + 32 * i, ch = tid & 7;
            *reinterpret_cast<u16x8_t*>(img + toff(row, ch)) = r[i];
        }
    }
};

// sum / max over the four 16-lane rows by VALU lane swaps (attention.hip)
__device__ __forceinline__ float pl16(float v, bool mx) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const float a = __uint_as_float(r[0]), b = __uint_as_float(r[1]);
    return mx ? fmaxf(a, b) : a + b;
}
__device__ __forceinline__ float pl32(float v, bool mx) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const float a = __uint_as_float(r[0]), b = __uint_as_float(r[1]);
    return mx ? fmaxf(a, b) : a + b;
}
__device__ __forceinline__ float rmax4(float v) { return pl32(pl16(v, true), true); }
__device__ __forceinline__ float rsum4(float v) { return pl32(pl16(v, false), false); }

__device__ __forceinline__ int clamp_len(int p, int Tmax) { return min(max(p, 0), Tmax); }

__global__ void __launch_bounds__(NTA) attn_extend_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ kcache,
                                                          const bf16_t* __restrict__ vcache, const int* __restrict__ lens,
                                                          bf16_t* __restrict__ out, int Tq, int H, int Tmax, float scale) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[2][2][64 * HD];     // [buf][K|V]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
    const int nqt = Tq / TILE;
    const int t = blockIdx.x, HB = gridDim.x / nqt;         // 1-D grid of nqt x H x B blocks, late query tiles first
    const int r_ = t / HB, hb = t - r_ * HB;
    const int qt = nqt - 1 - r_, h = hb % H, b = hb / H;
    const int D = H * HD;
    const long ld = 3L * D;
    const int p0 = __builtin_amdgcn_readfirstlane(clamp_len(lens[b], Tmax));
    const bf16_t* Kc = kcache + ((long)b * H + h) * Tmax * HD;
    const bf16_t* Vc = vcache + ((long)b * H + h) * Tmax * HD;
    const int q0 = qt * TILE + 16 * w;                      // this wave's 16 queries (index inside the sequence's Tq rows)
    const bf16_t* Q = qkv + ((long)b * Tq + q0) * ld + h * HD;
    const float c = scale * LOG2E;
    // limits (the last visible key): of the block, of the wave's first and last query, of this lane's query
    const int blast = min(p0 + qt * TILE + TILE - 1, Tmax - 1);
    const int wfirst = min(p0 + q0, Tmax - 1), wlast = min(p0 + q0 + 15, Tmax - 1);
    const int qlim = min(p0 + q0 + (lane & 15), Tmax - 1) - 4 * g;    // for key row 4 g + r of a fragment
    const int nkb = (blast >> 6) + 1;

    bf16x8_t qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = gfrag(Q, ld, ks, lane);

    f32x4_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;                           // key 0 is visible to every query: m is finite after tile 0

    constexpr int NOKEEP = 0x7fffffff;
    CacheTile ka, va, kn, vn;
    ka.load(Kc, 0, Tmax, NOKEEP, tid);
    va.load(Vc, 0, Tmax, blast, tid);
    ka.store(smem[0][0], tid);
    va.store(smem[0][1], tid);
    if (1 < nkb) {
        kn.load(Kc, 64, Tmax, NOKEEP, tid);
        vn.load(Vc, 64, Tmax, blast, tid);
    }
    __syncthreads();
    // tile kb is in LDS buffer cur = kb & 1; (hk, hv) hold tile kb + 1 in flight; (fk, fv) are free for kb + 2
    auto step = [&](const int kb, const int cur, CacheTile& hk, CacheTile& hv, CacheTile& fk, CacheTile& fv) {
        if (kb + 2 < nkb) {
            fk.load(Kc, (kb + 2) * 64, Tmax, NOKEEP, tid);
            fv.load(Vc, (kb + 2) * 64, Tmax, blast, tid);
        }
        const int k0 = kb * 64;
        if (k0 <= wlast) {                                  // wave-uniform: some query of the wave sees into this tile
            const bf16_t* Ki = smem[cur][0];
            const bf16_t* Vi = smem[cur][1];
            f32x4_t s[4];
#pragma unroll
            for (int kf = 0; kf < 4; ++kf) {
                const bf16x8_t a0 = frag_rows(Ki, 16 * kf, 0, lane), a1 = frag_rows(Ki, 16 * kf, 1, lane);
                f32x4_t z = {0.f, 0.f, 0.f, 0.f};
                z = mfma(a0, qf[0], z);
                s[kf] = mfma(a1, qf[1], z);
            }
            if (k0 + 63 > wfirst) {                         // wave-uniform: the tile reaches past the first query's limit
                const int lim = qlim - k0;                  // key k0 + 16 kf + 4 g + r is visible iff 16 kf + r <= lim
#pragma unroll
                for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[kf][r] = 16 * kf + r > lim ? -INFINITY : s[kf][r];
            }
            float mx = -INFINITY;
#pragma unroll
            for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kf][r]);
            const float mt = rmax4(mx) * c;                 // scaled-score domain (c > 0)
            const bool moved = __any(mt > m + RESC);
            const float mn = moved ? fmaxf(m, mt) : m;
            const float alpha = moved ? __builtin_amdgcn_exp2f(m - mn) : 1.f;
            float rs = 0.f;
#pragma unroll
            for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(s[kf][r], c, -mn));
                    s[kf][r] = p;
                    rs += p;
                }
            l = l * alpha + rs;                             // this lane's partial; rows summed at the end
            m = mn;
            if (moved) {
#pragma unroll
                for (int df = 0; df < 4; ++df) o[df] *= alpha;
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const bf16x8_t pb = pack_acc(s[2 * kk], s[2 * kk + 1]);
#pragma unroll
                for (int df = 0; df < 4; ++df) o[df] = mfma(frag_tr_perm(Vi, 16 * df, kk, lane), pb, o[df]);
            }
        }
        if (kb + 1 < nkb) {
            hk.store(smem[cur ^ 1][0], tid);
            hv.store(smem[cur ^ 1][1], tid);
        }
        __syncthreads();
    };
    for (int kb = 0; kb < nkb; kb += 2) {                   // unrolled by 2: register stages are compile-time
        step(kb, 0, kn, vn, ka, va);
        if (kb + 1 < nkb) step(kb + 1, 1, ka, va, kn, vn);
    }
    // lane holds O^T[d = 16 df + 4 g + r][q = q0 + (lane & 15)]
    l = rsum4(l);
    const float inv = 1.f / l;
    bf16_t* op = out + ((long)b * Tq + q0 + (lane & 15)) * D + h * HD;
#pragma unroll
    for (int df = 0; df < 4; ++df) {
        u16x4_t v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = f2bf(o[df][r] * inv);
        *reinterpret_cast<u16x4_t*>(op + 16 * df + 4 * g) = v;
    }
}

// 16-byte units: (b, h, j, sub) with sub fastest, so the cache is written in whole contiguous rows
__global__ void __launch_bounds__(NTA) kv_cache_append_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kcache,
                                                              bf16_t* __restrict__ vcache, const int* __restrict__ lens,
                                                              int Tq, int H, int Tmax, long total) {
    const int D = H * HD;
    for (long i = (long)blockIdx.x * NTA + threadIdx.x; i < total; i += (long)gridDim.x * NTA) {
        const int sub = (int)(i & 7);
        const long r = i >> 3;
        const int j = (int)(r % Tq);
        const long bh = r / Tq;
        const int h = (int)(bh % H);
        const long b = bh / H;
        const long slot = (long)clamp_len(lens[b], Tmax) + j;
        if (slot >= Tmax) continue;
        const bf16_t* src = qkv + (b * Tq + j) * 3L * D + h * HD + sub * 8;
        const long dst = (bh * Tmax + slot) * HD + sub * 8;
        *reinterpret_cast<u16x8_t*>(kcache + dst) = *reinterpret_cast<const u16x8_t*>(src + D);
        *reinterpret_cast<u16x8_t*>(vcache + dst) = *reinterpret_cast<const u16x8_t*>(src + 2 * D);
    }
}
}  // namespace

// queries per block of pdnn_attn_extend: Tq must be a multiple of it
PDNN_API int pdnn_attn_extend_tile() { return TILE; }

// qkv [B*Tq][3*H*64] bf16, kcache / vcache [B][H][Tmax][64] bf16, lens int32 [B] (device): K and V of row b*Tq + j into
// slot lens[b] + j (a slot >= Tmax is not stored); lens is not changed
PDNN_API int pdnn_kv_cache_append(const bf16_t* qkv, bf16_t* kcache, bf16_t* vcache, const int* lens, int B, int Tq, int H,
                                  int Tmax, hipStream_t st) {
    if (B < 1 || Tq < 1 || H < 1 || Tmax < 1 || Tq % TILE != 0 || !qkv || !kcache || !vcache || !lens)
        return (int)hipErrorInvalidValue;
    const long total = (long)B * H * Tq * 8;
    hipLaunchKernelGGL(kv_cache_append_kernel, dim3(stream_grid(total, NTA)), dim3(NTA), 0, st, qkv, kcache, vcache, lens,
                       Tq, H, Tmax, total);
    PDNN_LAUNCH_RET;
}

// after pdnn_kv_cache_append of the same qkv on the same stream: out [B*Tq][H*64] bf16, query row b*Tq + j at position
// lens[b] + j over the cache keys 0 .. lens[b] + j
PDNN_API int pdnn_attn_extend(const bf16_t* qkv, const bf16_t* kcache, const bf16_t* vcache, const int* lens, bf16_t* out,
                              int B, int Tq, int H, int Tmax, float scale, hipStream_t st) {
    if (B < 1 || Tq < 1 || H < 1 || Tmax < 1 || Tq % TILE != 0 || !qkv || !kcache || !vcache || !lens || !out)
        return (int)hipErrorInvalidValue;
    const long nblk = (long)B * H * (Tq / TILE);
    if (nblk > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(attn_extend_kernel, dim3((unsigned)nblk), dim3(NTA), 0, st, qkv, kcache, vcache, lens, out, Tq, H,
                       Tmax, scale);
    PDNN_LAUNCH_RET;
}
