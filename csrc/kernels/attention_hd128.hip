// Fused attention for head dim 128 (the usual width of GPT-style models above ~1B parameters; build_gpt2(n_embd=1024,
// n_head=8)), bf16 operands, fp32 softmax / accumulation, on the gfx950 MFMA 16x16x32 bf16 instruction.  The sibling of
// attention.hip (head dim 64), which is not templated on the head dim: the register and LDS budget of a 128-wide head is
// a different one, so these are kernels of their own.  No packed-document mask and no dropout here (the Python side
// refuses both at this head dim), and generation stays on the d = 64 kernels.
//
// Contract shared with attention.hip: q, k, v are column blocks of qkv[B*T][3D] (D = H * 128, ld = 3D), o[B*T][D] and
// dqkv[B*T][3D] use the same packing, lse2[B][H][T] is fp32 in the base-2 scaled-score domain, T % 128 == 0, both
// `causal` values, heavy tiles first over the whole 1-D grid.
//
// LDS tile image: [64 rows][128] bf16, 256-byte rows = 16 chunks of 16 bytes, chunk c of row r stored at chunk
//   c ^ sw(r),  sw(r) = ((r & 7) << 1) | ((r >> 3) & 1)          (a bijection of r & 15 onto 0..15)
// Every row starts at bank 0, so without the swizzle each fragment read would hit one 16-byte bank group 16 times over.
//   * K-major read (frag_rows, ds_read_b128): the 16 lanes of a lane group read chunk c of 16 consecutive rows; sw takes
//     16 different values there, so they cover all 64 banks once.
//   * transposed read (frag_tr_perm, ds_read_b64_tr_b16): 32 lanes read 8 consecutive rows (4 g + q, g in {0, 1} or
//     {2, 3}) x 32 bytes (the aligned chunk pair 2 df, 2 df + 1); sw puts the pair of row r at pair df ^ (r & 7), eight
//     different pairs = 256 bytes, all 64 banks once (bit 0 of sw only swaps the two chunks inside a pair).
//   * tile store (ds_write_b128): 16 lanes write the 16 chunks of one row, a permutation of one 256-byte line.
// This is by construction; no bank-conflict counter was read.
//
// Forward (attn128_fwd_kernel): one block = 128 queries of one (b, h), 4 waves x 32 queries, 64-key K and V tiles.
//   A K + V tile pair is 32 KB, so double-buffered staging is 64 KB: two blocks per CU fit the 160 KB of LDS, and two
//   blocks per CU (2 waves / SIMD) is also what the registers allow: O^T is 64 fp32 VGPRs per lane, the Q fragments 32,
//   the scores of a tile 32, and the ONE register stage of the next tile 32 (the d = 64 forward keeps two stages in
//   flight; here that would be 64 VGPRs, and a tile's 64 MFMAs per wave are twice the d = 64 cover for one load round
//   trip).  S^T = K Q^T takes four k-steps of 32; online softmax per query with the lazy rescale (RESC); P^T goes
//   from the accumulator registers straight into the B operand of O^T += V^T P^T, V^T read with ds_read_b64_tr_b16 in
//   the same permuted key order (no LDS round trip of P); one barrier per tile.
// Backward (FlashAttention-2 split, P recomputed from lse2, no atomics: results repeat bit for bit), one 16-row
// fragment per wave (NF = 1): with two, dK / dV would hold 128 accumulator VGPRs + 64 of K / V fragments before any
// score, and dQ 64 + 64 + 64 of scores; both spill.
//   attn128_bwd_dq_kernel:   one block = 64 queries (4 waves x 16), two passes over the 64-key tiles k <= query:
//       pass 0: S^T = K Q^T, P^T, dP^T = V dO^T, delta = sum_k P dP in fp32 (each lane 16 keys of every 64, the four
//               lane groups of a query combined by two lane swaps), written for the dK / dV kernel;
//       pass 1: the same S^T, P^T, dP^T again, dS^T = P^T (dP^T - delta), dQ^T += K^T dS^T.
//       delta is NOT rowsum(dO . O) from the forward's O, as the d = 64 kernels form it: O is stored in bf16, and its
//       rounding moves delta by up to 2^-9 sum_i |dO_i O_i|, a sum over the head dim that every dS of the row inherits.
//       Against the float64 reference that put dQ at 1.07 - 2.93 x the bound of the unfused chain (whose delta is
//       sum_k P dP too) in five of the six test cases, and the d = 64 kernels' dQ at 1.906 x.  sum_k P dP from the
//       unrounded P is the same quantity to fp32 accuracy; it costs pass 0, 32 of a tile's 48 MFMAs a second time
//       (backward 88 -> 110 us and 110 -> 139 us at B8 T1024 D768 / D1024), and `out` is no longer read.
//   attn128_bwd_dkdv_kernel, which runs after it: one block = 64 keys (4 waves x 16), loop over 64-query tiles q >= key:
//       S = Q K^T, P, dV^T += dO^T P, dP = dO V^T, dS = P (dP - delta), dK^T += Q^T dS; the tile's lse2 / delta ride
//       through LDS with its Q / dO tile.  The transposed fragments of a k-step are issued in two halves of eight
//       (all sixteen at once are 64 VGPRs).
//   An NF = 1 wave reads 1 KB of LDS per MFMA, which is the LDS rate at the MFMA rate: the backward is expected to be
//   LDS-bound, as the d = 64 NF = 1 kernels were.  A 128-query x 32-key dQ tile (two fragments per wave at half the
//   score registers) is the follow-up that would halve it.
//
// Build figures (hipcc -O3, VGPR-form MFMA, no packed fp32 VALU; profiles/attention_hd128.txt):
//   kernel                    VGPRs  AGPRs  scratch  LDS bytes  blocks / CU (waves / SIMD)
//   attn128_fwd_kernel          242      0        0      65536  2 (2): 2 x 64 KB of the 160 KB, 2 x 242 <= 512 VGPRs
//   attn128_bwd_dq_kernel       244      0        0      65536  2 (2)
//   attn128_bwd_dkdv_kernel     240      0        0      66560  2 (2)
//
// Numerics (tests/test_attn_hd128_gpu.py, worst error / bound over its six cases against the float64 chain reference
// with the chain's own constants, on an MI355X): y 0.77, dV 0.85, dQ 0.47, dK 0.50, lse2 0.03.
#include "common.h"

namespace {
constexpr int HD = 128;         // head dim
constexpr int NTA = 256;
constexpr int KT = 64;          // rows of one LDS tile (keys in the forward and dQ, queries in dK / dV)
constexpr float RESC = 8.f;     // forward lazy-rescale threshold (log2 units)
constexpr float LOG2E = 1.4426950408889634f;

// (tile, head, sequence) of this block of the 1-D grid of ntile x H x B blocks; the heaviest tiles come first over the
// whole grid (the dispatcher hands out blocks in index order, so the causal triangle's tail is short)
__device__ __forceinline__ void attn_block(int ntile, int H, bool heavy_is_last, int& tile, int& h, int& b) {
    const int t = blockIdx.x, HB = gridDim.x / ntile;
    const int r = t / HB, hb = t - r * HB;
    tile = heavy_is_last ? ntile - 1 - r : r;
    h = hb % H;
    b = hb / H;
}

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// [64][128] bf16 tile image, 256-byte rows, 16-byte chunk c of row r at chunk c ^ sw(r) (see the header)
__device__ __forceinline__ int toff(int row, int chunk) {
    const int sw = ((row & 7) << 1) | ((row >> 3) & 1);
    return row * HD + ((chunk ^ sw) << 3);
}

// K-major fragment: lane -> row (row0 + (lane & 15)), k = 32 ks + 8 (lane >> 4) .. +7
__device__ __forceinline__ bf16x8_t frag_rows(const bf16_t* img, int row0, int ks, int lane) {
    const int row = row0 + (lane & 15);
    return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(img + toff(row, ks * 4 + (lane >> 4))));
}

// Transposed fragment for an MFMA step over 32 tile rows [32 kk, 32 kk + 32) in the permuted order of an
// accumulator-sourced operand: lane (col = col0 + (lane & 15), group g) receives rows 32 kk + 4 g + 0..3 (elements 0-3)
// and 32 kk + 16 + 4 g + 0..3 (elements 4-7) of column col.
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

// 64 x 128 tile: 256 threads x 4 chunks; 16 lanes move one 256-byte row
struct TileLd {
    u16x8_t r[4];
    __device__ __forceinline__ void load(const bf16_t* src, long ld, int tid) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (tid >> 4) + 16 * i, ch = tid & 15;
            r[i] = *reinterpret_cast<const u16x8_t*>(src + (long)row * ld + ch * 8);
        }
    }
    __device__ __forceinline__ void store(bf16_t* img, int tid) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (tid >> 4) + 16 * i, ch = tid & 15;
            *reinterpret_cast<u16x8_t*>(img + toff(row, ch)) = r[i];
        }
    }
};

// max / sum over the four 16-lane rows (lanes l, l^16, l^32, l^48) by VALU lane swaps (no LDS round trip)
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

// ---------------------------------------------------------------------------------------------- forward
__global__ void __launch_bounds__(NTA) attn128_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                          float* __restrict__ lse2, int T, int H, float scale,
                                                          int causal) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[2][2][KT * HD];     // [buf][K|V], 64 KB
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
    const int nqb = T / 128;
    int qb, h, b;
    attn_block(nqb, H, true, qb, h, b);              // heavy (late) query tiles first
    const int D = H * HD;
    const long ld = 3L * D;
    const bf16_t* Q = qkv + (long)b * T * ld + h * HD;
    const bf16_t* Kp = Q + D;
    const bf16_t* Vp = Q + 2 * D;
    const int q0 = qb * 128 + 32 * w;                // this wave's 32 queries
    const float c = scale * LOG2E;

    bf16x8_t qf[2][4];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[f][ks] = gfrag(Q + (long)(q0 + 16 * f) * ld, ld, ks, lane);

    f32x4_t o[8][2];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) o[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // a wave's first tile (keys 0..63) holds a visible key for every query, so the maximum is finite after it
    float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};

    const int nkb = causal ? (qb * 128 + 128) / KT : T / KT;
    // tile kb is in LDS buffer kb & 1 while tile kb + 1 is in flight in (tk, tv): prefetch distance 1
    TileLd tk, tv;
    tk.load(Kp, ld, tid);
    tv.load(Vp, ld, tid);
    tk.store(smem[0][0], tid);
    tv.store(smem[0][1], tid);
    __syncthreads();
    for (int kb = 0; kb < nkb; ++kb) {
        const int cur = kb & 1;
        const bool more = kb + 1 < nkb;
        if (more) {
            tk.load(Kp + (long)(kb + 1) * KT * ld, ld, tid);
            tv.load(Vp + (long)(kb + 1) * KT * ld, ld, tid);
        }
        const int k0 = kb * KT;
        if (!causal || k0 <= q0 + 31) {              // wave-uniform: tile not entirely above the diagonal
            const bf16_t* Ki = smem[cur][0];
            const bf16_t* Vi = smem[cur][1];
            // S^T[key = k0 + 16 kf + 4 g + r][query = q0 + 16 f + (lane & 15)]
            f32x4_t s[4][2];
#pragma unroll
            for (int kf = 0; kf < 4; ++kf) {
                bf16x8_t a[4];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) a[ks] = frag_rows(Ki, 16 * kf, ks, lane);
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    f32x4_t z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) z = mfma(a[ks], qf[f][ks], z);
                    s[kf][f] = z;
                }
            }
            if (causal && k0 + KT - 1 > q0) {        // wave-uniform: only diagonal tiles need the mask
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    const int qi = q0 + 16 * f + (lane & 15);
#pragma unroll
                    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (k0 + 16 * kf + 4 * g + r > qi) s[kf][f][r] = -INFINITY;
                }
            }
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                float mx = -INFINITY;
#pragma unroll
                for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kf][f][r]);
                // lazy rescale: the running maximum moves only when some query's tile maximum exceeds it by more than
                // RESC; below that the tile's P values use the stale maximum (P <= 2^RESC, exact after the final 1 / l)
                const float mt = rmax4(mx) * c;                     // scaled-score domain (c > 0)
                const bool moved = __any(mt > m[f] + RESC);
                const float mn = moved ? fmaxf(m[f], mt) : m[f];
                const float alpha = moved ? __builtin_amdgcn_exp2f(m[f] - mn) : 1.f;
                float rs = 0.f;
#pragma unroll
                for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(s[kf][f][r], c, -mn));
                        s[kf][f][r] = p;
                        rs += p;
                    }
                l[f] = l[f] * alpha + rs;                           // this lane's partial; rows summed at the end
                m[f] = mn;
                if (moved) {
#pragma unroll
                    for (int df = 0; df < 8; ++df) o[df][f] *= alpha;
                }
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8_t pb[2];
#pragma unroll
                for (int f = 0; f < 2; ++f) pb[f] = pack_acc(s[2 * kk][f], s[2 * kk + 1][f]);
#pragma unroll
                for (int df = 0; df < 8; ++df) {
                    const bf16x8_t vfr = frag_tr_perm(Vi, 16 * df, kk, lane);
#pragma unroll
                    for (int f = 0; f < 2; ++f) o[df][f] = mfma(vfr, pb[f], o[df][f]);
                }
            }
        }
        if (more) {                                  // buffer cur ^ 1 was last read before the previous barrier
            tk.store(smem[cur ^ 1][0], tid);
            tv.store(smem[cur ^ 1][1], tid);
        }
        __syncthreads();
    }
    // lane holds O^T[d = 16 df + 4 g + r][q = q0 + 16 f + (lane & 15)]
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int qi = q0 + 16 * f + (lane & 15);
        l[f] = rsum4(l[f]);
        const float inv = 1.f / l[f];
        bf16_t* op = out + ((long)b * T + qi) * D + h * HD;
#pragma unroll
        for (int df = 0; df < 8; ++df) {
            u16x4_t v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = f2bf(o[df][f][r] * inv);
            *reinterpret_cast<u16x4_t*>(op + 16 * df + 4 * g) = v;
        }
        if (g == 0) lse2[((long)b * H + h) * T + qi] = m[f] + __log2f(l[f]);
    }
}

// ---------------------------------------------------------------------------------------------- backward
// dQ for 64 queries per block (wave w: queries q0 = 64 qb + 16 w .. + 15); loop over 64-key tiles; writes delta
__global__ void __launch_bounds__(NTA) attn128_bwd_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dO,
                                                             const float* __restrict__ lse2, float* __restrict__ delta,
                                                             bf16_t* __restrict__ dqkv, int T, int H, float scale,
                                                             int causal) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[2][2][KT * HD];     // [buf][K|V], 64 KB
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
    const int nqb = T / 64;
    int qb, h, b;
    attn_block(nqb, H, true, qb, h, b);
    const int D = H * HD;
    const long ld = 3L * D;
    const bf16_t* Q = qkv + (long)b * T * ld + h * HD;
    const bf16_t* Kp = Q + D;
    const bf16_t* Vp = Q + 2 * D;
    const bf16_t* dOp = dO + (long)b * T * D + h * HD;
    const int q0 = qb * 64 + 16 * w;
    const int ql = q0 + (lane & 15);
    const float c = scale * LOG2E;
    const float lq = lse2[((long)b * H + h) * T + ql];
    float dl = 0.f;                                  // pass 0: this lane's part of delta; pass 1: delta of query ql

    bf16x8_t qf[4], of[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        qf[ks] = gfrag(Q + (long)q0 * ld, ld, ks, lane);
        of[ks] = gfrag(dOp + (long)q0 * D, D, ks, lane);
    }
    f32x4_t dq[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) dq[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nkb = causal ? qb + 1 : T / KT;
    TileLd tk, tv;
    // pass 0 walks the key tiles for delta = sum_k P dP alone, pass 1 walks them again for dQ
    for (int pass = 0; pass < 2; ++pass) {
    tk.load(Kp, ld, tid);
    tv.load(Vp, ld, tid);
    tk.store(smem[0][0], tid);                       // every read of the pass before ended at its last barrier
    tv.store(smem[0][1], tid);
    __syncthreads();
    for (int kb = 0; kb < nkb; ++kb) {
        const int cur = kb & 1;
        const bool more = kb + 1 < nkb;
        if (more) {
            tk.load(Kp + (long)(kb + 1) * KT * ld, ld, tid);
            tv.load(Vp + (long)(kb + 1) * KT * ld, ld, tid);
        }
        const int k0 = kb * KT;
        if (!causal || k0 <= q0 + 15) {
            const bf16_t* Ki = smem[cur][0];
            const bf16_t* Vi = smem[cur][1];
            // S^T[key][q], dP^T[key][q]: lane holds rows key = k0 + 16 ki + 4 g + r, column q = ql
            f32x4_t s[4], dp[4];
#pragma unroll
            for (int ki = 0; ki < 4; ++ki) {
                f32x4_t z = {0.f, 0.f, 0.f, 0.f}, y = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    z = mfma(frag_rows(Ki, 16 * ki, ks, lane), qf[ks], z);
                    y = mfma(frag_rows(Vi, 16 * ki, ks, lane), of[ks], y);
                }
                s[ki] = z;
                dp[ki] = y;
            }
            const bool diag = causal && k0 + KT - 1 > q0;   // wave-uniform: only these tiles need the mask
#pragma unroll
            for (int ki = 0; ki < 4; ++ki) {
#pragma unroll
                for (int r = 0; r < 4; ++r) s[ki][r] = __builtin_amdgcn_exp2f(fmaf(s[ki][r], c, -lq));
                if (diag) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k0 + 16 * ki + 4 * g + r > ql) s[ki][r] = 0.f;
                }
                if (pass == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) dl = fmaf(s[ki][r], dp[ki][r], dl);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) dp[ki][r] = s[ki][r] * (dp[ki][r] - dl);
                }
            }
            if (pass == 1) {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const bf16x8_t sb = pack_acc(dp[2 * kk], dp[2 * kk + 1]);
                    bf16x8_t fk[8];              // the k-step's fragments issued before the MFMAs that use them
#pragma unroll
                    for (int df = 0; df < 8; ++df) fk[df] = frag_tr_perm(Ki, 16 * df, kk, lane);
#pragma unroll
                    for (int df = 0; df < 8; ++df) dq[df] = mfma(fk[df], sb, dq[df]);
                }
            }
        }
        if (more) {
            tk.store(smem[cur ^ 1][0], tid);
            tv.store(smem[cur ^ 1][1], tid);
        }
        __syncthreads();
    }
    if (pass == 0) {                                 // the four lane groups of query ql hold 16 keys of every 64 each
        dl = rsum4(dl);
        if (g == 0) delta[((long)b * H + h) * T + ql] = dl;
    }
    }
    // lane holds dQ^T[d = 16 df + 4 g + r][q = ql]
    bf16_t* dqp = dqkv + ((long)b * T + ql) * ld + h * HD;
#pragma unroll
    for (int df = 0; df < 8; ++df) {
        u16x4_t a;
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = f2bf(dq[df][r] * scale);
        *reinterpret_cast<u16x4_t*>(dqp + 16 * df + 4 * g) = a;
    }
}

// dK, dV for 64 keys per block (wave w: keys k0 = 64 kb + 16 w .. + 15); loop over 64-query tiles
__global__ void __launch_bounds__(NTA) attn128_bwd_dkdv_kernel(const bf16_t* __restrict__ qkv,
                                                               const bf16_t* __restrict__ dO,
                                                               const float* __restrict__ lse2,
                                                               const float* __restrict__ delta,
                                                               bf16_t* __restrict__ dqkv, int T, int H, float scale,
                                                               int causal) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[2][2][KT * HD];     // [buf][Q|dO], 64 KB
    __shared__ __attribute__((aligned(16))) float lsd[2][2][KT];             // [buf][lse2|delta][query], 1 KB
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
    const int nkb = T / 64;
    int kb, h, b;
    attn_block(nkb, H, false, kb, h, b);             // early key tiles have the most work: launched first
    const int D = H * HD;
    const long ld = 3L * D;
    const bf16_t* Q = qkv + (long)b * T * ld + h * HD;
    const bf16_t* Kp = Q + D;
    const bf16_t* Vp = Q + 2 * D;
    const bf16_t* dOp = dO + (long)b * T * D + h * HD;
    const float* L2 = lse2 + ((long)b * H + h) * T;
    const float* Dl = delta + ((long)b * H + h) * T;
    const int k0 = kb * 64 + 16 * w;
    const int kl = k0 + (lane & 15);
    const float c = scale * LOG2E;

    bf16x8_t kf[4], vf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        kf[ks] = gfrag(Kp + (long)k0 * ld, ld, ks, lane);
        vf[ks] = gfrag(Vp + (long)k0 * ld, ld, ks, lane);
    }
    f32x4_t dv[8], dk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) dv[i] = dk[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int qb0 = causal ? kb : 0;                 // first query tile that reaches this block's first key
    const int nqb = T / KT;
    // threads 0-15 move the tile's lse2, 16-31 its delta (one float4 each)
    const float* lsrc = tid < 16 ? L2 + 4 * tid : Dl + 4 * (tid & 15);
    float4 lrow = {0.f, 0.f, 0.f, 0.f};
    TileLd tq, tdo;
    tq.load(Q + (long)qb0 * KT * ld, ld, tid);
    tdo.load(dOp + (long)qb0 * KT * D, D, tid);
    if (tid < 32) lrow = *reinterpret_cast<const float4*>(lsrc + qb0 * KT);
    tq.store(smem[0][0], tid);
    tdo.store(smem[0][1], tid);
    if (tid < 32) *reinterpret_cast<float4*>(&lsd[0][tid >> 4][4 * (tid & 15)]) = lrow;
    __syncthreads();
    for (int qb = qb0; qb < nqb; ++qb) {
        const int cur = (qb - qb0) & 1;
        const bool more = qb + 1 < nqb;
        if (more) {
            tq.load(Q + (long)(qb + 1) * KT * ld, ld, tid);
            tdo.load(dOp + (long)(qb + 1) * KT * D, D, tid);
            if (tid < 32) lrow = *reinterpret_cast<const float4*>(lsrc + (qb + 1) * KT);
        }
        const int qs = qb * KT;
        if (!causal || qs + KT - 1 >= k0) {
            const bf16_t* Qi = smem[cur][0];
            const bf16_t* Oi = smem[cur][1];
            // S[q][key], dP[q][key]: lane holds rows q = qs + 16 qi + 4 g + r, column key = kl
            f32x4_t s[4], dp[4];
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) {
                f32x4_t z = {0.f, 0.f, 0.f, 0.f}, y = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    z = mfma(frag_rows(Qi, 16 * qi, ks, lane), kf[ks], z);
                    y = mfma(frag_rows(Oi, 16 * qi, ks, lane), vf[ks], y);
                }
                s[qi] = z;
                dp[qi] = y;
            }
            const bool diag = causal && qs < k0 + 16;       // wave-uniform: only these tiles need the mask
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) {
                const int qr = qs + 16 * qi + 4 * g;
                const float4 lv = *reinterpret_cast<const float4*>(&lsd[cur][0][16 * qi + 4 * g]);
                const float4 dd = *reinterpret_cast<const float4*>(&lsd[cur][1][16 * qi + 4 * g]);
                const float la[4] = {lv.x, lv.y, lv.z, lv.w}, da[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) s[qi][r] = __builtin_amdgcn_exp2f(fmaf(s[qi][r], c, -la[r]));
                if (diag) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kl > qr + r) s[qi][r] = 0.f;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) dp[qi][r] = s[qi][r] * (dp[qi][r] - da[r]);
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const bf16x8_t pb = pack_acc(s[2 * kk], s[2 * kk + 1]);
                const bf16x8_t sb = pack_acc(dp[2 * kk], dp[2 * kk + 1]);
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {     // eight transposed fragments at a time, issued before their MFMAs
                    bf16x8_t fo[4], fq[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        fo[j] = frag_tr_perm(Oi, 16 * (4 * hf + j), kk, lane);
                        fq[j] = frag_tr_perm(Qi, 16 * (4 * hf + j), kk, lane);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        dv[4 * hf + j] = mfma(fo[j], pb, dv[4 * hf + j]);
                        dk[4 * hf + j] = mfma(fq[j], sb, dk[4 * hf + j]);
                    }
                }
            }
        }
        if (more) {
            tq.store(smem[cur ^ 1][0], tid);
            tdo.store(smem[cur ^ 1][1], tid);
            if (tid < 32) *reinterpret_cast<float4*>(&lsd[cur ^ 1][tid >> 4][4 * (tid & 15)]) = lrow;
        }
        __syncthreads();
    }
    // lane holds dK^T / dV^T [d = 16 df + 4 g + r][key = kl]
    bf16_t* dkp = dqkv + ((long)b * T + kl) * ld + D + h * HD;
    bf16_t* dvp = dkp + D;
#pragma unroll
    for (int df = 0; df < 8; ++df) {
        u16x4_t a, v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            a[r] = f2bf(dk[df][r] * scale);
            v[r] = f2bf(dv[df][r]);
        }
        *reinterpret_cast<u16x4_t*>(dkp + 16 * df + 4 * g) = a;
        *reinterpret_cast<u16x4_t*>(dvp + 16 * df + 4 * g) = v;
    }
}
}  // namespace

// B, T, H >= 1, T % 128 == 0, no null pointer, and a grid (T / 64) H B that fits an int; else nothing is launched
static bool attn128_ok(int B, int T, int H, bool ptrs) {
    return B >= 1 && T >= 1 && H >= 1 && T % 128 == 0 && ptrs && (long)(T / 64) * H * B <= 0x7fffffffL;
}

// qkv [B*T][3*H*128] bf16 -> out [B*T][H*128] bf16, lse2 [B][H][T] fp32.  T % 128 == 0.
PDNN_API int pdnn_flash_attn_hd128_fwd(const bf16_t* qkv, bf16_t* out, float* lse2, int B, int T, int H, float scale,
                                       int causal, hipStream_t st) {
    if (!attn128_ok(B, T, H, qkv && out && lse2)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(attn128_fwd_kernel, dim3(T / 128 * H * B), dim3(NTA), 0, st, qkv, out, lse2, T, H, scale, causal);
    PDNN_LAUNCH_RET;
}

// dO [B*T][H*128], out / lse2 from the forward -> dqkv [B*T][3*H*128]; delta: fp32 [B][H][T] scratch, written by the dQ
// kernel and read by the dK / dV kernel behind it on the stream.  `out` must be given, as for the d = 64 entry, but is not
// read (see the header: delta comes from P and dP).
PDNN_API int pdnn_flash_attn_hd128_bwd(const bf16_t* qkv, const bf16_t* out, const bf16_t* dO, const float* lse2,
                                       float* delta, bf16_t* dqkv, int B, int T, int H, float scale, int causal,
                                       hipStream_t st) {
    if (!attn128_ok(B, T, H, qkv && out && dO && lse2 && delta && dqkv)) return (int)hipErrorInvalidValue;
    const dim3 grid(T / 64 * H * B);
    hipLaunchKernelGGL(attn128_bwd_dq_kernel, grid, dim3(NTA), 0, st, qkv, dO, lse2, delta, dqkv, T, H, scale, causal);
    hipLaunchKernelGGL(attn128_bwd_dkdv_kernel, grid, dim3(NTA), 0, st, qkv, dO, lse2, delta, dqkv, T, H, scale, causal);
    PDNN_LAUNCH_RET;
}
