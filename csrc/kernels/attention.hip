// Fused causal attention for head dim 64 (GPT-2; SURVEY.md §2.8 K-18 "flash-style attention"), bf16
// operands, fp32 softmax/accumulation, on the gfx950 MFMA 16x16x32 bf16 instruction.
//
// Layout: q, k, v are column blocks of the packed c_attn output qkv[B*T][3D] (ld = 3D): head h of
// token t of sequence b lives at row b*T + t, columns h*64 (q), D + h*64 (k), 2D + h*64 (v).  The output
// o[B*T][D] and the gradient dqkv[B*T][3D] use the same packing, so no head split/merge copies exist.
//
// Forward (one block = 128 queries of one (b, h), 4 waves x 32 queries; K/V tiles of 64 keys
// register-staged into double-buffered LDS, one barrier per tile):
//   S^T = K Q^T  ->  lane holds S^T[key = 16f + 4g + r][query = lane & 15]  (g = lane >> 4)
//   online softmax per query (= per lane; the 4 lane groups are combined by two xor-shuffles)
//   O^T += V^T P^T: P^T is consumed straight from the accumulator registers as the B operand of the
//   next MFMA (cdna_hip_programming.md §3 "An accumulator tile as the next MFMA's operand"); the k order
//   inside an MFMA step is permuted (element e of lane group g = key 4g + e or 16 + 4g + e - 4), and the
//   V^T operand is read with ds_read_b64_tr_b16 from exactly those permuted key rows, so no LDS round trip
//   of P is needed.
// Saves lse2 = m + log2(sum) (base-2, scaled-score domain) per query for the backward.
//
// Backward (FlashAttention-2 split, both kernels recompute P from lse2):
//   attn_bwd_dkdv: one block = 64 keys (4 waves x 16 keys), loop over query tiles q >= key:
//       S = Q K^T, P, dV^T += dO^T P, dP = dO V^T, dS = P (dP - delta), dK^T += Q^T dS
//   attn_bwd_dq:   one block = 64 queries (4 waves x 16 queries), loop over key tiles k <= query:
//       S^T = K Q^T, P^T, dP^T = V dO^T, dS^T, dQ^T += K^T dS^T
//   delta[q] = sum_d dO[q][d] O[q][d] comes from attn_bwd_delta.
//
// Packed documents (template parameter DOC; the plain instantiations compile to the code they had before it existed,
// profiles/attention_doc_mask.txt): query q of sequence b sees key k iff doc_start[b][q] <= k <= q.  doc_start[b][t] is
// the first token of t's document, doc_end[b][t] one past its last; both int32 [B][T], non-decreasing in t, and every
// value is clamped into [0, T] before it becomes a tile index or an address (a malformed array gives wrong numbers,
// never an out-of-range access).  Tile ranges follow the bounds from both sides: the key loops of the forward and of
// dQ start at the tile of the block's first doc_start, a wave skips a tile wholly before the doc_start of its first
// query, and the document mask runs only on "edge" tiles (k0 < doc_start of the wave's last query; wave-uniform, like
// diag).  The query loop of dK / dV ends at the tile of the doc_end of the block's last key, a wave skips a tile at or
// past the doc_end of its last key, and masks only tiles that reach the doc_end of its first key.  On an edge tile of
// the forward a query may have every key masked while its running maximum is still -inf (queries 96..127 with documents
// starting at 60 and 100: query 100 in key tile 0); the DOC forward therefore starts the maximum at a finite floor
// (see there), which gives p = 0 with l and m unchanged on such a tile and costs no tile anything.
// The block order stays heavy-causal-first (late query tiles, early key tiles).  With short documents that is no longer
// the order of decreasing work (a late query tile may hold one short document); a work-sorted order is left for a
// measured follow-up.
#include "common.h"
#include "dropout_rng.h"
#include "tuning.h"

// Block order over (query or key tile, head, sequence): 0 = 3-D grid, heavy tiles first inside each (head, sequence);
// 1 = 1-D grid, heavy tiles first over the WHOLE grid (the dispatcher hands out blocks in index order, so the last
// blocks to start are the lightest ones and the causal triangle's tail is short)
#ifndef PDNN_ATTN_ORDER
#define PDNN_ATTN_ORDER 1
#endif

namespace {
constexpr int HD = 64;          // head dim

// (tile, head, sequence) of this block; heavy = tile index giving the most work first
__device__ __forceinline__ void attn_block(int ntile, int H, bool heavy_is_last, int& tile, int& h, int& b) {
#if PDNN_ATTN_ORDER == 1
    const int t = blockIdx.x, HB = gridDim.x / ntile;      // 1-D grid of ntile x H x B blocks
    const int r = t / HB, hb = t - r * HB;
    tile = heavy_is_last ? ntile - 1 - r : r;
    h = hb % H;
    b = hb / H;
#else
    tile = heavy_is_last ? ntile - 1 - (int)blockIdx.x : (int)blockIdx.x;
    h = blockIdx.y;
    b = blockIdx.z;
#endif
}
constexpr int NTA = 256;

// the last kernel argument: ``int causal`` of the plain kernels, the two bound arrays of the DOC ones
struct DocArg {
    const int* start;           // doc_start [B][T]
    const int* end;             // doc_end [B][T]
};
// DROP: the same with the dropout argument behind it, so the plain and DOC kernels keep the signature they had
struct CausalDrop {
    int causal;
    pdrop::Arg drop;
};
struct DocDrop {
    DocArg doc;
    pdrop::Arg drop;
};
template <bool DOC, bool DROP = false> struct MaskSel { typedef int type; };
template <> struct MaskSel<true, false> { typedef DocArg type; };
template <> struct MaskSel<false, true> { typedef CausalDrop type; };
template <> struct MaskSel<true, true> { typedef DocDrop type; };
__device__ __forceinline__ int mask_causal(int causal) { return causal; }
__device__ __forceinline__ int mask_causal(const DocArg&) { return 1; }
__device__ __forceinline__ int mask_causal(const CausalDrop& m) { return m.causal; }
__device__ __forceinline__ int mask_causal(const DocDrop&) { return 1; }
__device__ __forceinline__ const DocArg& mask_doc(const DocArg& m) { return m; }
__device__ __forceinline__ const DocArg& mask_doc(const DocDrop& m) { return m.doc; }
// this block's dropout stream: key of (state, site, b * H + h), and x0 = k0 + q * (T / 4) of a query row
struct DropCtx {
    uint32_t k0, k1, thr;
    float scale;
};
template <typename M>
__device__ __forceinline__ DropCtx drop_ctx(const M& m, int b, int h, int H) {
    const pdrop::Key k = pdrop::stream_key(m.drop.state, m.drop.site, (uint32_t)(b * H + h));
    return DropCtx{k.k0, k.k1, m.drop.thr, m.drop.scale};
}
__device__ __forceinline__ DropCtx drop_ctx(int, int, int, int) { return DropCtx{0u, 0u, 0u, 1.f}; }
__device__ __forceinline__ DropCtx drop_ctx(const DocArg&, int, int, int) { return DropCtx{0u, 0u, 0u, 1.f}; }
__device__ __forceinline__ int clamp_t(int v, int T) { return min(max(v, 0), T); }
constexpr float RESC = 8.f;     // forward lazy-rescale threshold (log2 units)
constexpr float LOG2E = 1.4426950408889634f;

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// [64][64] bf16 tile image, 128-byte rows, 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7)
__device__ __forceinline__ int toff(int row, int chunk) { return row * HD + ((chunk ^ ((row >> 1) & 7)) << 3); }

// K-major fragment: lane -> row (row0 + (lane & 15)), k = 32 ks + 8 (lane >> 4) .. +7
__device__ __forceinline__ bf16x8_t frag_rows(const bf16_t* img, int row0, int ks, int lane) {
    const int row = row0 + (lane & 15);
    return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(img + toff(row, ks * 4 + (lane >> 4))));
}

// Transposed fragment for an MFMA step over 32 tile rows [32 kk, 32 kk + 32) in the permuted order of
// an accumulator-sourced operand: lane (col = col0 + (lane & 15), group g) receives rows
// 32kk + 4g + 0..3 (elements 0-3) and 32kk + 16 + 4g + 0..3 (elements 4-7) of column col.
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

// 64 x 64 tile: 256 threads x 2 chunks
struct TileLd {
    u16x8_t r[2];
    __device__ __forceinline__ void load(const bf16_t* src, long ld, int tid) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (tid >> 3) + 32 * i, ch = tid & 7;
            r[i] = *reinterpret_cast<const u16x8_t*>(src + (long)row * ld + ch * 8);
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

// max / sum over the four 16-lane rows (lanes l, l^16, l^32, l^48) by VALU lane swaps: v_permlane16_swap /
// v_permlane32_swap with both operands v return (v, partner) in some order per lane, so combining the pair is
// the xor-16 / xor-32 step (no ds_bpermute round trip through the LDS pipe)
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
// DROP: l and lse2 come from the undropped P (the softmax is unchanged); only the P packed into the P V operand is
// masked, and 1 / (1 - p) rides on the final 1 / l
template <bool DOC, bool DROP>
__global__ void __launch_bounds__(NTA) attn_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                       float* __restrict__ lse2, int T, int H, float scale,
                                                       typename MaskSel<DOC, DROP>::type mk) {
    const int causal = mask_causal(mk);
    __shared__ __attribute__((aligned(16))) bf16_t smem[2][2][64 * HD];     // [buf][K|V]
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

    bf16x8_t qf[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[f][ks] = gfrag(Q + (long)(q0 + 16 * f) * ld, ld, ks, lane);

    f32x4_t o[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) o[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // DOC: the running maximum starts at a finite floor, not -inf.  A plain wave's first tile holds a visible key for
    // every query (key 0 is in tile 0); with documents it need not (queries 96..127, documents from 60 and 100: query
    // 100 has key tile 0 fully masked), and with m = -inf that tile would form exp2(fmaf(-inf, c, +inf)) = NaN.  From the
    // floor the same tile gives p = exp2(-inf) = 0 and alpha = exp2(0) = 1: l and m unchanged, at no cost on any tile;
    // the first visible key then moves m exactly as from -inf (alpha = exp2(floor - m) = 0 on l = 0, O = 0).
    constexpr float M0 = DOC ? -3.0e38f : -INFINITY;
    float m[2] = {M0, M0}, l[2] = {0.f, 0.f};

    const int nkb = causal ? (qb * 128 + 128) / 64 : T / 64;
    // DOC: first key tile of the block, doc_start of the wave's first / last query (wave-uniform), of this lane's queries
    int kb0 = 0, ws_first = 0, ws_last = 0, dsl[2] = {0, 0};
    if constexpr (DOC) {
        const int* ds = mask_doc(mk).start + (long)b * T;
        kb0 = min(clamp_t(ds[qb * 128], T) >> 6, nkb - 1);
        ws_first = __builtin_amdgcn_readfirstlane(clamp_t(ds[q0], T));
        ws_last = __builtin_amdgcn_readfirstlane(clamp_t(ds[q0 + 31], T));
#pragma unroll
        for (int f = 0; f < 2; ++f) dsl[f] = clamp_t(ds[q0 + 16 * f + (lane & 15)], T) - 4 * g;    // for key row 4 g + r
    }
    // DROP: x of the word of (this lane's query of fragment f, key granule g of tile 0): + (k0 >> 2) + 4 kf per word
    const DropCtx dc = drop_ctx(mk, b, h, H);
    uint32_t dx0[2] = {0u, 0u};
    if constexpr (DROP) {
#pragma unroll
        for (int f = 0; f < 2; ++f) dx0[f] = dc.k0 + (uint32_t)(q0 + 16 * f + (lane & 15)) * (uint32_t)(T >> 2) + g;
    }
    // K/V tiles: prefetch distance 2 (two register stages + two LDS buffers).  The per-tile compute of a
    // d=64 head is short, so with distance 1 every iteration waited out most of a global-load round trip
    // (causal and full attention took the same time: latency-, not throughput-bound).
    TileLd ka, va, kn, vn;
    ka.load(Kp + (long)kb0 * 64 * ld, ld, tid);
    va.load(Vp + (long)kb0 * 64 * ld, ld, tid);
    ka.store(smem[0][0], tid);
    va.store(smem[0][1], tid);
    if (kb0 + 1 < nkb) {
        kn.load(Kp + (long)(kb0 + 1) * 64 * ld, ld, tid);
        vn.load(Vp + (long)(kb0 + 1) * 64 * ld, ld, tid);
    }
    __syncthreads();
    // tile kb is in LDS buffer cur = (kb - kb0) & 1; (hk, hv) hold tile kb + 1 in flight; (fk, fv) are free for kb + 2
    auto step = [&](const int kb, const int cur, TileLd& hk, TileLd& hv, TileLd& fk, TileLd& fv) {
        if (kb + 2 < nkb) {
            fk.load(Kp + (long)(kb + 2) * 64 * ld, ld, tid);
            fv.load(Vp + (long)(kb + 2) * 64 * ld, ld, tid);
        }
        const int k0 = kb * 64;
        // wave-uniform: tile not entirely above the diagonal (DOC: nor entirely before the wave's first document)
        if ((!causal || k0 <= q0 + 31) && (!DOC || k0 + 63 >= ws_first)) {
            const bf16_t* Ki = smem[cur][0];
            const bf16_t* Vi = smem[cur][1];
            f32x4_t s[4][2];
#pragma unroll
            for (int kf = 0; kf < 4; ++kf) {
                const bf16x8_t a0 = frag_rows(Ki, 16 * kf, 0, lane), a1 = frag_rows(Ki, 16 * kf, 1, lane);
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    f32x4_t z = {0.f, 0.f, 0.f, 0.f};
                    z = mfma(a0, qf[f][0], z);
                    s[kf][f] = mfma(a1, qf[f][1], z);
                }
            }
            // VALU budget per tile is what bounds a d=64 head (32 MFMAs vs ~32 softmax elements per lane):
            // the causal mask runs only on diagonal tiles (wave-uniform branch), the softmax scale is folded
            // into the exponent's FMA, exp2 is the raw v_exp_f32 (arguments <= 0; underflow to 0 is
            // exactly what softmax wants), and O is rescaled only when some row maximum moved.
            const bool diag = causal && k0 + 63 > q0;
            if (diag) {
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
            if constexpr (DOC) {
                if (k0 < ws_last) {                  // wave-uniform "edge": some query's document starts inside or after
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        const int lim = dsl[f] - k0;        // key k0 + 16 kf + 4 g + r is before the document
#pragma unroll
                        for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (16 * kf + r < lim) s[kf][f][r] = -INFINITY;
                    }
                }
            }
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                float mx = -INFINITY;
#pragma unroll
                for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kf][f][r]);
                // lazy rescale (cdna_hip_programming.md T13): the running maximum moves only when some query's tile
                // maximum exceeds it by more than 2^RESC in probability terms; below that the tile's P values use
                // the stale maximum (P <= 2^RESC, exact after the final 1 / l) and O and l keep their scale
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
                if constexpr (DROP) {                               // after the row sum: l stays the undropped one
#pragma unroll
                    for (int kf = 0; kf < 4; ++kf) {
                        const uint32_t wd = pdrop::word_x(dx0[f] + (uint32_t)((k0 >> 2) + 4 * kf), dc.k1);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (!pdrop::keep(wd, r, dc.thr)) s[kf][f][r] = 0.f;
                    }
                }
                if (moved) {
#pragma unroll
                    for (int df = 0; df < 4; ++df) o[df][f] *= alpha;
                }
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8_t pb[2];
#pragma unroll
                for (int f = 0; f < 2; ++f) pb[f] = pack_acc(s[2 * kk][f], s[2 * kk + 1][f]);
#pragma unroll
                for (int df = 0; df < 4; ++df) {
                    const bf16x8_t vfr = frag_tr_perm(Vi, 16 * df, kk, lane);
#pragma unroll
                    for (int f = 0; f < 2; ++f) o[df][f] = mfma(vfr, pb[f], o[df][f]);
                }
            }
        }
        if (kb + 1 < nkb) {
            hk.store(smem[cur ^ 1][0], tid);
            hv.store(smem[cur ^ 1][1], tid);
        }
        __syncthreads();
    };
    for (int kb = kb0; kb < nkb; kb += 2) {          // unrolled by 2: register stages are compile-time
        step(kb, 0, kn, vn, ka, va);
        if (kb + 1 < nkb) step(kb + 1, 1, ka, va, kn, vn);
    }
    // lane holds O^T[d = 16 df + 4 g + r][q = q0 + 16 f + (lane & 15)]
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int qi = q0 + 16 * f + (lane & 15);
        l[f] = rsum4(l[f]);
        const float inv = DROP ? dc.scale / l[f] : 1.f / l[f];
        bf16_t* op = out + ((long)b * T + qi) * D + h * HD;
#pragma unroll
        for (int df = 0; df < 4; ++df) {
            u16x4_t v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = f2bf(o[df][f][r] * inv);
            *reinterpret_cast<u16x4_t*>(op + 16 * df + 4 * g) = v;
        }
        if (g == 0) lse2[((long)b * H + h) * T + qi] = m[f] + __log2f(l[f]);
    }
}

// ---------------------------------------------------------------------------------------------- backward
// delta[b][h][t] = sum_d dO . O   (one thread per (row, head), 8 x 16-byte loads each)
__global__ void __launch_bounds__(NTA) attn_bwd_delta_kernel(const bf16_t* __restrict__ o, const bf16_t* __restrict__ dO,
                                                             float* __restrict__ delta, int BT, int T, int H) {
    const long i = (long)blockIdx.x * NTA + threadIdx.x;
    if (i >= (long)BT * H) return;
    const long row = i / H;
    const int h = (int)(i - row * H);
    const int D = H * HD;
    const bf16_t* a = o + row * D + h * HD;
    const bf16_t* bb = dO + row * D + h * HD;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float x[8], y[8];
        unpack8(*reinterpret_cast<const u16x8_t*>(a + 8 * c), x);
        unpack8(*reinterpret_cast<const u16x8_t*>(bb + 8 * c), y);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += x[j] * y[j];
    }
    const long bidx = row / T, t = row - bidx * T;
    delta[(bidx * H + h) * T + t] = s;
}

// dK, dV for 64 NF keys per block (wave w: NF 16-key fragments from k0 = 64 NF kb + 16 NF w); loop over 64-query
// tiles.  NF = 2 reads every Q / dO fragment out of LDS once for two key fragments (see attn_bwd_dq_kernel).
// DROP: dV^T += dO^T (P o keep), scaled by 1 / (1 - p) at the end; dS = P (keep dP / (1 - p) - delta)
template <int NF, bool DOC, bool DROP>
__global__ void __launch_bounds__(NTA) attn_bwd_dkdv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dO,
                                                            const float* __restrict__ lse2, const float* __restrict__ delta,
                                                            bf16_t* __restrict__ dqkv, int T, int H, float scale,
                                                            typename MaskSel<DOC, DROP>::type mk) {
    const int causal = mask_causal(mk);
    __shared__ __attribute__((aligned(16))) bf16_t smem[2][2][64 * HD];     // [buf][Q|dO]
    // the query tile's lse2 / delta ride along with its Q / dO tile through LDS: loaded from global memory in the
    // compute loop they were waited on behind the next tile's prefetch loads (vmcnt is in order), every tile
    __shared__ __attribute__((aligned(16))) float lsd[2][2][64];              // [buf][lse2|delta][query]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
    const int nkb = T / (64 * NF);
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
    const int k0 = kb * 64 * NF + 16 * NF * w;
    const float c = scale * LOG2E;

    bf16x8_t kf[NF][2], vf[NF][2];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kf[f][ks] = gfrag(Kp + (long)(k0 + 16 * f) * ld, ld, ks, lane);
            vf[f][ks] = gfrag(Vp + (long)(k0 + 16 * f) * ld, ld, ks, lane);
        }
    f32x4_t dv[NF][4], dk[NF][4];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int i = 0; i < 4; ++i) dv[f][i] = dk[f][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int qb0 = causal ? kb * NF : 0;            // first query tile that reaches this block's first key
    int nqb = T / 64;
    // DOC: the query loop ends with the document of the block's last key; doc_end of the wave's first / last key
    // (wave-uniform) and of this lane's keys
    int we_first = 0, we_last = 0, del[NF];
    if constexpr (DOC) {
        const int* de = mask_doc(mk).end + (long)b * T;
        nqb = max(min((clamp_t(de[kb * 64 * NF + 64 * NF - 1], T) + 63) >> 6, nqb), qb0 + 1);
        we_first = __builtin_amdgcn_readfirstlane(clamp_t(de[k0], T));
        we_last = __builtin_amdgcn_readfirstlane(clamp_t(de[k0 + 16 * NF - 1], T));
#pragma unroll
        for (int f = 0; f < NF; ++f) del[f] = clamp_t(de[k0 + 16 * f + (lane & 15)], T) - 4 * g;   // for query row 4 g + r
    }
    // DROP: this lane's keys are element (kl & 3) of granule kl >> 2; x of query 4 g of tile 0, + (qs + 16 qi + r) T / 4
    const DropCtx dc = drop_ctx(mk, b, h, H);
    uint32_t dx0[NF];
    if constexpr (DROP) {
#pragma unroll
        for (int f = 0; f < NF; ++f)
            dx0[f] = dc.k0 + (uint32_t)((k0 + 16 * f + (lane & 15)) >> 2) + (uint32_t)(4 * g) * (uint32_t)(T >> 2);
    }
    const int dj = 8 * (lane & 3);                   // key & 3 = lane & 3: the byte of the word
    // threads 0-15 move the tile's lse2, 16-31 its delta (one float4 each)
    const float* lsrc = tid < 16 ? L2 + 4 * tid : Dl + 4 * (tid - 16);
    float4 lrow = {0.f, 0.f, 0.f, 0.f};
    TileLd tq, tdo;
    tq.load(Q + (long)qb0 * 64 * ld, ld, tid);
    tdo.load(dOp + (long)qb0 * 64 * D, D, tid);
    if (tid < 32) lrow = *reinterpret_cast<const float4*>(lsrc + qb0 * 64);
    tq.store(smem[0][0], tid);
    tdo.store(smem[0][1], tid);
    if (tid < 32) *reinterpret_cast<float4*>(&lsd[0][tid >> 4][4 * (tid & 15)]) = lrow;
    // every prologue load (the K / V fragments above included) has landed: no wait for them inside the loop,
    // where the compiler's in-order vmcnt waits would otherwise also wait out the next tile's prefetch
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    for (int qb = qb0; qb < nqb; ++qb) {
        const int cur = (qb - qb0) & 1;
        const bool more = qb + 1 < nqb;
        if (more) {
            tq.load(Q + (long)(qb + 1) * 64 * ld, ld, tid);
            tdo.load(dOp + (long)(qb + 1) * 64 * D, D, tid);
            if (tid < 32) lrow = *reinterpret_cast<const float4*>(lsrc + (qb + 1) * 64);
        }
        const int qs = qb * 64;
        if ((!causal || qs + 63 >= k0) && (!DOC || qs < we_last)) {
            const bf16_t* Qi = smem[cur][0];
            const bf16_t* Oi = smem[cur][1];
            // S[q][key], dP[q][key]: lane holds rows q = qs + 16 qi + 4 g + r, column key = k0 + 16 f + (lane & 15)
            f32x4_t s[NF][4], dp[NF][4];
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) {
                const bf16x8_t q0f = frag_rows(Qi, 16 * qi, 0, lane), q1f = frag_rows(Qi, 16 * qi, 1, lane);
                const bf16x8_t o0f = frag_rows(Oi, 16 * qi, 0, lane), o1f = frag_rows(Oi, 16 * qi, 1, lane);
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    f32x4_t z = {0.f, 0.f, 0.f, 0.f};
                    z = mfma(q0f, kf[f][0], z);
                    s[f][qi] = mfma(q1f, kf[f][1], z);
                    f32x4_t y = {0.f, 0.f, 0.f, 0.f};
                    y = mfma(o0f, vf[f][0], y);
                    dp[f][qi] = mfma(o1f, vf[f][1], y);
                }
            }
            const bool diag = causal && qs < k0 + 16 * NF;  // wave-uniform: only these tiles need the mask
            const bool edge = DOC && qs + 63 >= we_first;   // wave-uniform: the tile reaches past some key's document
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) {
                const int qr = qs + 16 * qi + 4 * g;
                const float4 lv = *reinterpret_cast<const float4*>(&lsd[cur][0][16 * qi + 4 * g]);
                const float4 dl = *reinterpret_cast<const float4*>(&lsd[cur][1][16 * qi + 4 * g]);
                const float la[4] = {lv.x, lv.y, lv.z, lv.w}, da[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    const int kl = k0 + 16 * f + (lane & 15);
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[f][qi][r] = __builtin_amdgcn_exp2f(fmaf(s[f][qi][r], c, -la[r]));
                    if (diag) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (kl > qr + r) s[f][qi][r] = 0.f;
                    }
                    if constexpr (DOC) {
                        if (edge) {
                            const int lim = del[f] - qs;    // query qs + 16 qi + 4 g + r is past the document
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (16 * qi + r >= lim) s[f][qi][r] = 0.f;
                        }
                    }
                    if constexpr (DROP) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const uint32_t wd = pdrop::word_x(dx0[f] + (uint32_t)(qs + 16 * qi + r) * (uint32_t)(T >> 2), dc.k1);
                            const bool kp = ((wd >> dj) & 255u) >= dc.thr;
                            const float pr = s[f][qi][r];
                            dp[f][qi][r] = pr * ((kp ? dp[f][qi][r] * dc.scale : 0.f) - da[r]);
                            s[f][qi][r] = kp ? pr : 0.f;
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) dp[f][qi][r] = s[f][qi][r] * (dp[f][qi][r] - da[r]);
                    }
                }
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8_t pb[NF], sb[NF];
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    pb[f] = pack_acc(s[f][2 * kk], s[f][2 * kk + 1]);
                    sb[f] = pack_acc(dp[f][2 * kk], dp[f][2 * kk + 1]);
                }
                // all eight transposed fragments of this k-step issued before the MFMAs that use them (one at a
                // time, every MFMA waited out its own LDS read)
                bf16x8_t fo[4], fq[4];
#pragma unroll
                for (int df = 0; df < 4; ++df) {
                    fo[df] = frag_tr_perm(Oi, 16 * df, kk, lane);
                    fq[df] = frag_tr_perm(Qi, 16 * df, kk, lane);
                }
#pragma unroll
                for (int df = 0; df < 4; ++df)
#pragma unroll
                    for (int f = 0; f < NF; ++f) {
                        dv[f][df] = mfma(fo[df], pb[f], dv[f][df]);
                        dk[f][df] = mfma(fq[df], sb[f], dk[f][df]);
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
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int kl = k0 + 16 * f + (lane & 15);
        bf16_t* dkp = dqkv + ((long)b * T + kl) * ld + D + h * HD;
        bf16_t* dvp = dkp + D;
#pragma unroll
        for (int df = 0; df < 4; ++df) {
            u16x4_t a, v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                a[r] = f2bf(dk[f][df][r] * scale);
                v[r] = f2bf(DROP ? dv[f][df][r] * dc.scale : dv[f][df][r]);
            }
            *reinterpret_cast<u16x4_t*>(dkp + 16 * df + 4 * g) = a;
            *reinterpret_cast<u16x4_t*>(dvp + 16 * df + 4 * g) = v;
        }
    }
}

// dQ for 64 NF queries per block (wave w: NF 16-query fragments from q0 = 64 NF qb + 16 NF w); loop over 64-key
// tiles.  NF = 2 reads every K / V fragment out of LDS once for two query fragments: at NF = 1 a wave's 24 MFMAs
// per tile came with 24 KB of LDS reads, which saturated the LDS array (256 B/clk/CU) at the MFMA rate.
// DELTA: the block also forms delta = rowsum(dO . O) of its queries (the four 16-lane groups of a query row take
// 16 dims each) and writes it for attn_bwd_dkdv_kernel, which then runs after it: no separate delta launch
// DROP: dS^T = P^T (keep dP^T / (1 - p) - delta); delta = rowsum(dO . O) already holds the dropout through O
template <bool DELTA, int NF, bool DOC, bool DROP>
__global__ void __launch_bounds__(NTA) attn_bwd_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dO,
                                                          const float* __restrict__ lse2, float* __restrict__ delta,
                                                          const bf16_t* __restrict__ o,
                                                          bf16_t* __restrict__ dqkv, int T, int H, float scale,
                                                          typename MaskSel<DOC, DROP>::type mk) {
    const int causal = mask_causal(mk);
    __shared__ __attribute__((aligned(16))) bf16_t smem[2][2][64 * HD];     // [buf][K|V]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
    const int nqb = T / (64 * NF);
    int qb, h, b;
    attn_block(nqb, H, true, qb, h, b);
    const int D = H * HD;
    const long ld = 3L * D;
    const bf16_t* Q = qkv + (long)b * T * ld + h * HD;
    const bf16_t* Kp = Q + D;
    const bf16_t* Vp = Q + 2 * D;
    const bf16_t* dOp = dO + (long)b * T * D + h * HD;
    const int q0 = qb * 64 * NF + 16 * NF * w;
    const float c = scale * LOG2E;
    int ql[NF];
    float lq[NF], dq_[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        ql[f] = q0 + 16 * f + (lane & 15);
        lq[f] = lse2[((long)b * H + h) * T + ql[f]];
        if constexpr (DELTA) {
            const long ro = ((long)b * T + ql[f]) * D + h * HD + 16 * g;
            float sd = 0.f;
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) {
                float x[8], y[8];
                unpack8(*reinterpret_cast<const u16x8_t*>(o + ro + 8 * c2), x);
                unpack8(*reinterpret_cast<const u16x8_t*>(dO + ro + 8 * c2), y);
#pragma unroll
                for (int j = 0; j < 8; ++j) sd += x[j] * y[j];
            }
            sd = rsum4(sd);
            dq_[f] = sd;
            if (g == 0) delta[((long)b * H + h) * T + ql[f]] = sd;
        } else {
            dq_[f] = delta[((long)b * H + h) * T + ql[f]];
        }
    }

    bf16x8_t qf[NF][2], of[NF][2];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[f][ks] = gfrag(Q + (long)(q0 + 16 * f) * ld, ld, ks, lane);
            of[f][ks] = gfrag(dOp + (long)(q0 + 16 * f) * D, D, ks, lane);
        }
    f32x4_t dq[NF][4];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int i = 0; i < 4; ++i) dq[f][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nkb = causal ? (qb + 1) * NF : T / 64;
    // DOC: as in the forward, per 16 NF-query wave
    int kb0 = 0, ws_first = 0, ws_last = 0, dsl[NF];
    if constexpr (DOC) {
        const int* ds = mask_doc(mk).start + (long)b * T;
        kb0 = min(clamp_t(ds[qb * 64 * NF], T) >> 6, nkb - 1);
        ws_first = __builtin_amdgcn_readfirstlane(clamp_t(ds[q0], T));
        ws_last = __builtin_amdgcn_readfirstlane(clamp_t(ds[q0 + 16 * NF - 1], T));
#pragma unroll
        for (int f = 0; f < NF; ++f) dsl[f] = clamp_t(ds[ql[f]], T) - 4 * g;       // for key row 4 g + r
    }
    const DropCtx dc = drop_ctx(mk, b, h, H);        // DROP: as in the forward
    uint32_t dx0[NF];
    if constexpr (DROP) {
#pragma unroll
        for (int f = 0; f < NF; ++f) dx0[f] = dc.k0 + (uint32_t)ql[f] * (uint32_t)(T >> 2) + g;
    }
    TileLd tk, tv;
    tk.load(Kp + (long)kb0 * 64 * ld, ld, tid);
    tv.load(Vp + (long)kb0 * 64 * ld, ld, tid);
    tk.store(smem[0][0], tid);
    tv.store(smem[0][1], tid);
    __syncthreads();
    for (int kb = kb0; kb < nkb; ++kb) {
        const int cur = (kb - kb0) & 1;
        const bool more = kb + 1 < nkb;
        if (more) {
            tk.load(Kp + (long)(kb + 1) * 64 * ld, ld, tid);
            tv.load(Vp + (long)(kb + 1) * 64 * ld, ld, tid);
        }
        const int k0 = kb * 64;
        if ((!causal || k0 <= q0 + 16 * NF - 1) && (!DOC || k0 + 63 >= ws_first)) {
            const bf16_t* Ki = smem[cur][0];
            const bf16_t* Vi = smem[cur][1];
            // S^T[key][q], dP^T[key][q]: lane holds rows key = k0 + 16 ki + 4 g + r, column q = ql[f]
            f32x4_t s[NF][4], dp[NF][4];
#pragma unroll
            for (int ki = 0; ki < 4; ++ki) {
                const bf16x8_t k0f = frag_rows(Ki, 16 * ki, 0, lane), k1f = frag_rows(Ki, 16 * ki, 1, lane);
                const bf16x8_t v0f = frag_rows(Vi, 16 * ki, 0, lane), v1f = frag_rows(Vi, 16 * ki, 1, lane);
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    f32x4_t z = {0.f, 0.f, 0.f, 0.f};
                    z = mfma(k0f, qf[f][0], z);
                    s[f][ki] = mfma(k1f, qf[f][1], z);
                    f32x4_t y = {0.f, 0.f, 0.f, 0.f};
                    y = mfma(v0f, of[f][0], y);
                    dp[f][ki] = mfma(v1f, of[f][1], y);
                }
            }
            const bool diag = causal && k0 + 63 > q0;     // wave-uniform: only these tiles need the mask
            const bool edge = DOC && k0 < ws_last;        // wave-uniform: some query's document starts inside or after
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int ki = 0; ki < 4; ++ki) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[f][ki][r] = __builtin_amdgcn_exp2f(fmaf(s[f][ki][r], c, -lq[f]));
                    if (diag) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (k0 + 16 * ki + 4 * g + r > ql[f]) s[f][ki][r] = 0.f;
                    }
                    if constexpr (DOC) {
                        if (edge) {
                            const int lim = dsl[f] - k0;    // key k0 + 16 ki + 4 g + r is before the document
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (16 * ki + r < lim) s[f][ki][r] = 0.f;
                        }
                    }
                    if constexpr (DROP) {
                        const uint32_t wd = pdrop::word_x(dx0[f] + (uint32_t)((k0 >> 2) + 4 * ki), dc.k1);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            dp[f][ki][r] = s[f][ki][r] * ((pdrop::keep(wd, r, dc.thr) ? dp[f][ki][r] * dc.scale : 0.f) - dq_[f]);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) dp[f][ki][r] = s[f][ki][r] * (dp[f][ki][r] - dq_[f]);
                    }
                }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8_t sb[NF];
#pragma unroll
                for (int f = 0; f < NF; ++f) sb[f] = pack_acc(dp[f][2 * kk], dp[f][2 * kk + 1]);
                bf16x8_t fk[4];                  // fragments issued before the MFMAs (as in attn_bwd_dkdv)
#pragma unroll
                for (int df = 0; df < 4; ++df) fk[df] = frag_tr_perm(Ki, 16 * df, kk, lane);
#pragma unroll
                for (int df = 0; df < 4; ++df)
#pragma unroll
                    for (int f = 0; f < NF; ++f) dq[f][df] = mfma(fk[df], sb[f], dq[f][df]);
            }
        }
        if (more) {
            tk.store(smem[cur ^ 1][0], tid);
            tv.store(smem[cur ^ 1][1], tid);
        }
        __syncthreads();
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        bf16_t* dqp = dqkv + ((long)b * T + ql[f]) * ld + h * HD;
#pragma unroll
        for (int df = 0; df < 4; ++df) {
            u16x4_t a;
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = f2bf(dq[f][df][r] * scale);
            *reinterpret_cast<u16x4_t*>(dqp + 16 * df + 4 * g) = a;
        }
    }
}
// ---------------------------------------------------------------------------------------------- document bounds
// doc_start / doc_end of one sequence per block from its tokens: token t starts a document iff t == 0 or token t - 1
// is EOT (the EOT token belongs to the document it ends).  doc_start = prefix max of (start flag ? t : 0), doc_end =
// suffix min of (token t is EOT ? t + 1 : T).  Thread i owns the contiguous chunk [i n, i n + n), n = ceil(T / 256):
// chunk totals, a 256-entry scan in LDS, then the chunk again with the carry.
__global__ void __launch_bounds__(NTA) doc_bounds_kernel(const long long* __restrict__ idx, long long eot,
                                                         int* __restrict__ doc_start, int* __restrict__ doc_end, int T) {
    __shared__ int pmax[NTA], smin[NTA];
    const int tid = threadIdx.x;
    const long long* row = idx + (long)blockIdx.x * T;
    int* ds = doc_start + (long)blockIdx.x * T;
    int* de = doc_end + (long)blockIdx.x * T;
    const int n = (T + NTA - 1) / NTA;
    const int t0 = min(tid * n, T), t1 = min(t0 + n, T);
    int mx = 0, mn = T;
    for (int t = t0; t < t1; ++t) {
        if (t > 0 && row[t - 1] == eot) mx = t;
        if (row[t] == eot) mn = min(mn, t + 1);
    }
    pmax[tid] = mx;
    smin[tid] = mn;
    __syncthreads();
    for (int d = 1; d < NTA; d <<= 1) {
        const int a = tid >= d ? pmax[tid - d] : 0;
        const int e = tid + d < NTA ? smin[tid + d] : T;
        __syncthreads();
        pmax[tid] = max(pmax[tid], a);
        smin[tid] = min(smin[tid], e);
        __syncthreads();
    }
    int s = tid > 0 ? pmax[tid - 1] : 0;
    for (int t = t0; t < t1; ++t) {
        if (t > 0 && row[t - 1] == eot) s = t;
        ds[t] = s;
    }
    int e = tid + 1 < NTA ? smin[tid + 1] : T;
    for (int t = t1 - 1; t >= t0; --t) {
        if (row[t] == eot) e = t + 1;
        de[t] = e;
    }
}
}  // namespace

static dim3 attn_grid(int ntile, int H, int B) {
#if PDNN_ATTN_ORDER == 1
    return dim3(ntile * H * B);
#else
    return dim3(ntile, H, B);
#endif
}

template <bool DOC, bool DROP = false>
static void launch_fwd(const bf16_t* qkv, bf16_t* out, float* lse2, int B, int T, int H, float scale,
                       typename MaskSel<DOC, DROP>::type mk, hipStream_t st) {
    hipLaunchKernelGGL((attn_fwd_kernel<DOC, DROP>), attn_grid(T / 128, H, B), dim3(NTA), 0, st, qkv, out, lse2, T, H,
                       scale, mk);
}

// DOC at NF = 2 needs no scratch either (profiles/attention_doc_mask.txt), so attn_bwd_wide routes it like the plain
// one.  DROP always takes NF = 1: at NF = 2 the sixteen words per fragment pair bring dK / dV to 254 - 256 VGPRs (no
// scratch, but one wave / SIMD) and it measured slower than NF = 1 (profiles/attention_dropout.txt), so the NF = 2 DROP
// kernel is not instantiated
template <bool DOC, bool DROP = false>
static void launch_dkdv(const bf16_t* qkv, const bf16_t* dO, const float* lse2, const float* delta, bf16_t* dqkv, int B,
                        int T, int H, float scale, typename MaskSel<DOC, DROP>::type mk, hipStream_t st) {
    if constexpr (!DROP) {
        if (pg::tune().attn_bwd_wide & 2) {
            hipLaunchKernelGGL((attn_bwd_dkdv_kernel<2, DOC, false>), attn_grid(T / 128, H, B), dim3(NTA), 0, st, qkv, dO,
                               lse2, delta, dqkv, T, H, scale, mk);
            return;
        }
    }
    hipLaunchKernelGGL((attn_bwd_dkdv_kernel<1, DOC, DROP>), attn_grid(T / 64, H, B), dim3(NTA), 0, st, qkv, dO, lse2, delta,
                       dqkv, T, H, scale, mk);
}

template <bool DELTA, bool DOC, bool DROP = false>
static void launch_dq(const bf16_t* qkv, const bf16_t* out, const bf16_t* dO, const float* lse2, float* delta,
                      bf16_t* dqkv, int B, int T, int H, float scale, typename MaskSel<DOC, DROP>::type mk,
                      hipStream_t st) {
    if (pg::tune().attn_bwd_wide & 1)
        hipLaunchKernelGGL((attn_bwd_dq_kernel<DELTA, 2, DOC, DROP>), attn_grid(T / 128, H, B), dim3(NTA), 0, st, qkv, dO,
                           lse2, delta, out, dqkv, T, H, scale, mk);
    else
        hipLaunchKernelGGL((attn_bwd_dq_kernel<DELTA, 1, DOC, DROP>), attn_grid(T / 64, H, B), dim3(NTA), 0, st, qkv, dO,
                           lse2, delta, out, dqkv, T, H, scale, mk);
}

template <bool DOC, bool DROP = false>
static void launch_bwd(const bf16_t* qkv, const bf16_t* out, const bf16_t* dO, const float* lse2, float* delta,
                       bf16_t* dqkv, int B, int T, int H, float scale, typename MaskSel<DOC, DROP>::type mk,
                       hipStream_t st) {
    if (pg::tune().attn_delta_in_dq) {       // dQ first (it writes delta), then dK / dV
        launch_dq<true, DOC, DROP>(qkv, out, dO, lse2, delta, dqkv, B, T, H, scale, mk, st);
        launch_dkdv<DOC, DROP>(qkv, dO, lse2, delta, dqkv, B, T, H, scale, mk, st);
        return;
    }
    const long n = (long)B * T * H;
    hipLaunchKernelGGL(attn_bwd_delta_kernel, dim3((unsigned)((n + NTA - 1) / NTA)), dim3(NTA), 0, st, out, dO, delta,
                       B * T, T, H);
    launch_dkdv<DOC, DROP>(qkv, dO, lse2, delta, dqkv, B, T, H, scale, mk, st);
    launch_dq<false, DOC, DROP>(qkv, out, dO, lse2, delta, dqkv, B, T, H, scale, mk, st);
}

// The two entries.  One forward and one backward serve every variant; the optional arguments pick the kernels:
//   doc_start, doc_end  int32 [B][T] (pdnn_doc_bounds), both null (plain) or both given (packed documents, DOC)
//   p, state, site      dropout p on the probabilities (dropout_rng.h, DROP): p in [0, 1), quantised to thr / 256; state =
//                       device int64[2] (seed, step), read by the kernels; site >= 0; T <= 65536 keeps the granule index
//                       inside 32 bits.  p == 0 takes the kernels without DROP (they are faster): state may then be null
//                       and site is ignored.
// DOC and DROP exist under the causal mask only, so either with causal == 0 is refused; the plain kernels take ``causal``
// as it comes.  The backward takes what the forward took.  Anything refused returns hipErrorInvalidValue, nothing launched.
static bool attn_dims_ok(int B, int T, int H, bool ptrs) { return B >= 1 && T >= 1 && H >= 1 && T % 128 == 0 && ptrs; }

template <typename M> constexpr bool is_doc = std::is_same<M, DocArg>::value || std::is_same<M, DocDrop>::value;
template <typename M> constexpr bool is_drop = std::is_same<M, CausalDrop>::value || std::is_same<M, DocDrop>::value;

// calls f with the kernels' last argument (int causal, DocArg, CausalDrop or DocDrop); false, f not called, when refused
template <typename F>
static bool with_mask(int causal, const int* doc_start, const int* doc_end, float p, const long long* state, int site,
                      int T, F&& f) {
    if ((doc_start == nullptr) != (doc_end == nullptr) || ((doc_start || p != 0.f) && !causal)) return false;
    if (p == 0.f) {
        if (doc_start)
            f(DocArg{doc_start, doc_end});
        else
            f(causal);
        return true;
    }
    uint32_t thr;
    if (!pdrop::threshold(p, &thr) || !state || site < 0 || T > 65536) return false;
    const pdrop::Arg a{state, (uint32_t)site, thr, pdrop::scale_of(thr)};
    if (doc_start)
        f(DocDrop{DocArg{doc_start, doc_end}, a});
    else
        f(CausalDrop{1, a});
    return true;
}

// qkv [B*T][3*H*64] bf16 -> out [B*T][H*64] bf16, lse2 [B][H][T] fp32.  T % 128 == 0.
PDNN_API int pdnn_flash_attn_fwd(const bf16_t* qkv, bf16_t* out, float* lse2, int B, int T, int H, float scale,
                                 int causal, const int* doc_start, const int* doc_end, float p, const long long* state,
                                 int site, hipStream_t st) {
    if (!attn_dims_ok(B, T, H, qkv && out && lse2) ||
        !with_mask(causal, doc_start, doc_end, p, state, site, T, [&](auto mk) {
            using M = decltype(mk);
            launch_fwd<is_doc<M>, is_drop<M>>(qkv, out, lse2, B, T, H, scale, mk, st);
        }))
        return (int)hipErrorInvalidValue;
    PDNN_LAUNCH_RET;
}

// dO [B*T][H*64], out/lse2 from the forward -> dqkv [B*T][3*H*64]; delta: fp32 [B][H][T] scratch.
PDNN_API int pdnn_flash_attn_bwd(const bf16_t* qkv, const bf16_t* out, const bf16_t* dO, const float* lse2,
                                 float* delta, bf16_t* dqkv, int B, int T, int H, float scale, int causal,
                                 const int* doc_start, const int* doc_end, float p, const long long* state, int site,
                                 hipStream_t st) {
    if (!attn_dims_ok(B, T, H, qkv && out && dO && lse2 && delta && dqkv) ||
        !with_mask(causal, doc_start, doc_end, p, state, site, T, [&](auto mk) {
            using M = decltype(mk);
            launch_bwd<is_doc<M>, is_drop<M>>(qkv, out, dO, lse2, delta, dqkv, B, T, H, scale, mk, st);
        }))
        return (int)hipErrorInvalidValue;
    PDNN_LAUNCH_RET;
}

// idx int64 [B][T] -> doc_start, doc_end int32 [B][T]; one block per sequence, no host read-back (capturable)
PDNN_API int pdnn_doc_bounds(const long long* idx, long long eot, int* doc_start, int* doc_end, int B, int T,
                             hipStream_t st) {
    if (B < 1 || T < 1 || !idx || !doc_start || !doc_end) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(doc_bounds_kernel, dim3(B), dim3(NTA), 0, st, idx, eot, doc_start, doc_end, T);
    PDNN_LAUNCH_RET;
}
