// The fp8 (OCP e4m3fn) key/value cache of GPT-2 generation (generate(kv_cache="fp8")): the quantising cache writers and
// the decode, multi-query and extend attention kernels that read codes instead of bf16 rows.  Head dim 64.
//
// Format.  kcache, vcache uint8 [B][H][Tmax][64]: one 64-byte code row per (b, h, slot); kscale, vscale fp32
// [B][H][Tmax]: one power-of-two scale per row.  The rule is that of ops/quant.py (quantize_rows_reference) and of
// quant_rows_e4m3_kernel in gemm_skinny_fp8.hip, applied to one 64-element row: a = the largest bf16 magnitude of the
// row as its 15-bit pattern, e = (a >> 7) - 126 - (mantissa <= 96 ? 9 : 8) clamped to [-100, 100] (0 for a zero row),
// code = e4m3fn(x 2^-e) (v_cvt_pk_fp8_f32; the product is exact and at most 448), scale = 2^e.  dq = value(code) * scale
// is exactly a bf16 number.  lens int32 [B] on the device is read by the kernels and never written, and is clamped
// before it becomes an address, as in attention_decode.hip ([0, Tmax - 1]) and attention_extend.hip ([0, Tmax]).
// Slots at or past lens[b] may hold any byte and any scale (NaN included): they are never read before they are written.
//
// pdnn_kv_cache_fill_fp8 / pdnn_kv_cache_append_fp8: the twins of kv_cache_fill / kv_cache_append.  8 lanes own one row
// of K and the same row of V: 16 bytes (8 bf16) per lane and tensor, the row amax as an integer maximum over the 8 lanes
// by DPP (quad, quad pair, half row), 8 codes per lane, so the group stores the contiguous 64-byte code row, and lane 0
// of the group the two scales.  Append: slot = clamp(lens[b]) + j, a slot >= Tmax is not stored.
//
// pdnn_attn_decode_fp8 / pdnn_attn_decode_multi_fp8: attention_decode.hip's split over keys with its static grid
// B*H*ceil(Tmax / CHUNK), CHUNK in {64, 128, 256}, its partial format (o at part[blk][64], (m, l) behind them), its
// combine arithmetic (copied below), no atomics and fixed summation orders.  The thread layout is new: a code row is 64
// bytes, so 4 lanes share a key (16 dims = one 16-byte load each), a pass of 256 threads covers 64 keys, a chunk takes
// CHUNK / 64 passes and a wave reads 1 KiB of contiguous cache per load instruction.  All K and V codes and scales of
// the chunk are loaded before the first use.  v_cvt_scalef32_pk_f32_fp8 converts two codes with the row scale as its
// scale operand, so the fp32 operand of every FMA is exactly dq; q.k is 16 FMAs per lane in dim order, then the 4-lane
// DPP sum; P stays fp32; the 64 per-key-slot V accumulators go through LDS and are added in key-slot order by one wave.
// The new tokens (slots lens[b] .. lens[b] + S - 1): their 4 lanes read the bf16 k and v from qkv, quantise them in
// registers by the rule above (amax over the 4 lanes), store codes and scale (a slot >= Tmax is not stored) and use
// those same codes and scale in the arithmetic, so a key has one value in the step that creates it and in every later
// one.  Only slots < lens[b] are read from the cache; each new slot has one writer, the block whose chunk holds it.
// One kernel body serves both entries: the multi-query kernel loads the chunk once and runs the single-query
// arithmetic per query (phase 1: score rows and maxima; phase 2: P, l, o), so its output and cache equal S successive
// single-query calls bit for bit.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), CHUNK 64 / 128 / 256:
//   single query: VGPRs 48 / 62 / 84, LDS 16656 / 16912 / 17424 bytes, scratch 0
//   multi query:  VGPRs 47 / 74 / 118, LDS 18560 / 20608 / 24704 bytes, scratch 0
//   kv_cache_quant_kernel (fill and append): VGPRs 37, LDS 0, scratch 0
//
// pdnn_attn_extend_fp8: attention_extend.hip's forward with a converting stage.  The tile loader reads, per 16-byte LDS
// chunk, 8 codes and the row's scale, converts with v_cvt_scalef32_pk_bf16_fp8 and writes the same swizzled bf16 LDS
// image; everything behind the image is that kernel, copied (masking by select, V rows past the block's last visible
// key zeroed while staged, lazy rescale, MFMA order).  dq is exact in bf16, so the result equals pdnn_attn_extend on
// the dequantised cache bit for bit.
//   attn_extend_fp8_kernel: 94 VGPRs (0 AGPRs), 32768 bytes LDS, scratch 0, 5 waves / SIMD
#include "common.h"

namespace {
constexpr int HD = 64;              // head dim = bytes of a code row
constexpr int NTD = 256;            // threads per block
constexpr int KPP = NTD / 4;        // keys per pass of the decode kernels
constexpr int MAXS = 8;             // most queries per sequence of the multi-query kernel
constexpr float LOG2E = 1.4426950408889634f;

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

__device__ __forceinline__ int clamp_slot(int p, int Tmax) { return min(max(p, 0), Tmax - 1); }      // decode
__device__ __forceinline__ int clamp_len(int p, int Tmax) { return min(max(p, 0), Tmax); }           // append, extend

template <int CTRL>
__device__ __forceinline__ unsigned dpp_u(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}

// ------------------------------------------------------------------------------------------------ the row rule
__device__ __forceinline__ unsigned amax8(const u16x8_t& a, unsigned m) {
#pragma unroll
    for (int j = 0; j < 8; ++j) m = max(m, (unsigned)(a[j] & 0x7FFF));
    return m;
}

// a: the row's largest bf16 magnitude as its bit pattern -> e (frexp: m = (1 + mant / 128) / 2, x = E - 126;
// m <= 0.875 <=> mant <= 96; a subnormal clamps to -100)
__device__ __forceinline__ int row_exp(unsigned a) {
    if (!a) return 0;
    const int e = (int)(a >> 7) - 126 - ((a & 127) <= 96 ? 9 : 8);
    return min(max(e, -100), 100);
}
__device__ __forceinline__ float pow2(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }

// 8 bf16 times s = 2^-e -> 8 codes, element j in byte j
__device__ __forceinline__ uint2 codes8(const u16x8_t& a, float s) {
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(a[0]) * s, bf2f(a[1]) * s, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(a[2]) * s, bf2f(a[3]) * s, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(a[4]) * s, bf2f(a[5]) * s, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(a[6]) * s, bf2f(a[7]) * s, hi, true);
    return make_uint2((unsigned)lo, (unsigned)hi);
}

// ------------------------------------------------------------------------------------------------ fill / append
// 16-byte units of qkv: (b, h, j, sub) with sub fastest; the 8 lanes of a row are neighbours inside one 16-lane DPP row
template <bool APPEND>
__global__ void __launch_bounds__(NTD) kv_cache_quant_kernel(const bf16_t* __restrict__ qkv, uint8_t* __restrict__ kcache,
                                                             uint8_t* __restrict__ vcache, float* __restrict__ kscale,
                                                             float* __restrict__ vscale, const int* __restrict__ lens,
                                                             int T, int H, int Tmax, long total) {
    const int D = H * HD;
    for (long i = (long)blockIdx.x * NTD + threadIdx.x; i < total; i += (long)gridDim.x * NTD) {
        const int sub = (int)(i & 7);
        const long r = i >> 3;
        const int j = (int)(r % T);
        const long bh = r / T;
        const int h = (int)(bh % H);
        const long b = bh / H;
        const long slot = APPEND ? (long)clamp_len(lens[b], Tmax) + j : j;
        if (slot >= Tmax) continue;                         // the same for the 8 lanes of a row
        const bf16_t* src = qkv + (b * T + j) * 3L * D + h * HD + sub * 8;
        const u16x8_t kb = *reinterpret_cast<const u16x8_t*>(src + D);
        const u16x8_t vb = *reinterpret_cast<const u16x8_t*>(src + 2 * D);
        unsigned mk = amax8(kb, 0), mv = amax8(vb, 0);
        mk = max(mk, dpp_u<0xB1>(mk));
        mv = max(mv, dpp_u<0xB1>(mv));
        mk = max(mk, dpp_u<0x4E>(mk));
        mv = max(mv, dpp_u<0x4E>(mv));
        mk = max(mk, dpp_u<0x141>(mk));
        mv = max(mv, dpp_u<0x141>(mv));
        const int ek = row_exp(mk), ev = row_exp(mv);
        const long row = bh * Tmax + slot;
        *reinterpret_cast<uint2*>(kcache + row * HD + sub * 8) = codes8(kb, pow2(-ek));
        *reinterpret_cast<uint2*>(vcache + row * HD + sub * 8) = codes8(vb, pow2(-ev));
        if (sub == 0) {
            kscale[row] = pow2(ek);
            vscale[row] = pow2(ev);
        }
    }
}

// ------------------------------------------------------------------------------------------------ decode
// 16 codes and their row scale -> 16 fp32, exactly dq (the scale is a power of two)
__device__ __forceinline__ void cvt16(const u32x4_t& c, float sc, float* f) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const f32x2_t lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c[d], sc, false);
        const f32x2_t hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c[d], sc, true);
        f[4 * d] = lo[0];
        f[4 * d + 1] = lo[1];
        f[4 * d + 2] = hi[0];
        f[4 * d + 3] = hi[1];
    }
}

// the 4 lanes of a new key or value row: 16 bf16 each from qkv -> 16 codes and the row scale (amax over the 4 lanes)
__device__ __forceinline__ u32x4_t quant_new(const bf16_t* src, float& inv) {
    const u16x8_t a = *reinterpret_cast<const u16x8_t*>(src), b = *reinterpret_cast<const u16x8_t*>(src + 8);
    unsigned m = amax8(b, amax8(a, 0));
    m = max(m, dpp_u<0xB1>(m));
    m = max(m, dpp_u<0x4E>(m));
    const int e = row_exp(m);
    inv = pow2(e);
    const uint2 lo = codes8(a, pow2(-e)), hi = codes8(b, pow2(-e));
    return u32x4_t{lo.x, lo.y, hi.x, hi.y};
}

// sum over the 4 lanes that share a key; every lane of the 4 gets the total
__device__ __forceinline__ float sum4(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    return v;
}

// attention_decode.hip's chunk_tail over KPP = 64 key slots: by the threads tid < HD (one wave), l = sum of the chunk's P
// in ascending key order, o[tid] = sum over the key slots in order; the final bf16 row (one chunk) or the partial
template <int CHUNK>
__device__ __forceinline__ void chunk_tail(const float* sc, const float (*red)[HD], int tid, float m, bool direct,
                                           bf16_t* orow, float* po, float* pml) {
    float l = 0.f;
#pragma unroll 8
    for (int j = 0; j < CHUNK; ++j) l += sc[j];
    float o = 0.f;
#pragma unroll 8
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

// MS = 1: the single-query kernel (S == 1); MS = MAXS: S queries per sequence.  Partial of (row r = b*S + j, h, chunk
// ch) at index (r*H + h)*nchunk + ch.
template <int CHUNK, int MS>
__global__ void __launch_bounds__(NTD) attn_decode_fp8_kernel(const bf16_t* __restrict__ qkv, uint8_t* __restrict__ kcache,
                                                              uint8_t* __restrict__ vcache, float* __restrict__ kscale,
                                                              float* __restrict__ vscale, const int* __restrict__ lens,
                                                              bf16_t* __restrict__ out, float* __restrict__ part, int S_,
                                                              int H, int Tmax, int nchunk, float scale) {
    constexpr int NP = CHUNK / KPP;                         // passes
    __shared__ float sc[MS][CHUNK];                         // per query: scaled scores, then P
    __shared__ __attribute__((aligned(16))) float red[KPP][HD];
    __shared__ float wred[MS][NTD / 64];
    const int S = MS == 1 ? 1 : S_;
    const int tid = threadIdx.x, slot = tid >> 2, sub = tid & 3;
    const int blk = blockIdx.x, ch = blk % nchunk, bh = blk / nchunk, h = bh % H, b = bh / H;
    const int p0 = clamp_slot(lens[b], Tmax);               // query j sits at p0 + j
    const int k0 = ch * CHUNK;
    const int D = H * HD;
    const long npart = (long)gridDim.x * S;
    const bf16_t* qrow0 = qkv + (long)b * S * 3 * D + h * HD + sub * 16;
    uint8_t* Kc = kcache + (long)bh * Tmax * HD + sub * 16;
    uint8_t* Vc = vcache + (long)bh * Tmax * HD + sub * 16;
    float* Ks = kscale + (long)bh * Tmax;
    float* Vs = vscale + (long)bh * Tmax;
    u32x4_t kr[NP], vr[NP];
    float ksc[NP], vsc[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int key = k0 + i * KPP + slot;
        kr[i] = u32x4_t{0, 0, 0, 0};                        // code 0 with scale 1: a key nobody sees is +0
        vr[i] = u32x4_t{0, 0, 0, 0};
        ksc[i] = 1.f;
        vsc[i] = 1.f;
        if (key < p0) {
            kr[i] = *reinterpret_cast<const u32x4_t*>(Kc + (long)key * HD);
            vr[i] = *reinterpret_cast<const u32x4_t*>(Vc + (long)key * HD);
            ksc[i] = Ks[key];
            vsc[i] = Vs[key];
        } else if (key - p0 < S) {                          // new token key - p0 (its 4 lanes): from qkv, quantised here
            const bf16_t* r = qrow0 + (long)(key - p0) * 3 * D;
            kr[i] = quant_new(r + D, ksc[i]);
            vr[i] = quant_new(r + 2 * D, vsc[i]);
            if (key < Tmax) {
                *reinterpret_cast<u32x4_t*>(Kc + (long)key * HD) = kr[i];
                *reinterpret_cast<u32x4_t*>(Vc + (long)key * HD) = vr[i];
                if (sub == 0) {
                    Ks[key] = ksc[i];
                    Vs[key] = vsc[i];
                }
            }
        }
    }
    const float c = scale * LOG2E;
    for (int j = 0; j < S; ++j) {                           // phase 1; every branch on j is block-uniform
        const int p = p0 + j;
        if (k0 > p) continue;
        float q[16];
        unpack8(*reinterpret_cast<const u16x8_t*>(qrow0 + (long)j * 3 * D), q);
        unpack8(*reinterpret_cast<const u16x8_t*>(qrow0 + (long)j * 3 * D + 8), q + 8);
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int key = k0 + i * KPP + slot;
            float kf[16], s = 0.f;
            cvt16(kr[i], ksc[i], kf);
#pragma unroll
            for (int e = 0; e < 16; ++e) s = fmaf(q[e], kf[e], s);
            s = sum4(s) * c;
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
        if (k0 > p) {                                       // nothing visible to this query in this chunk: neutral partial
            if (tid < HD) po[tid] = 0.f;
            if (tid == 0) {
                pml[0] = -INFINITY;
                pml[1] = 0.f;
            }
            continue;
        }
        const float m = fmaxf(fmaxf(wred[j][0], wred[j][1]), fmaxf(wred[j][2], wred[j][3]));      // finite: key k0 <= p
        float acc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const float pk = __builtin_amdgcn_exp2f(sc[j][i * KPP + slot] - m);          // exp2(-inf) = 0 past p
            if (sub == 0) sc[j][i * KPP + slot] = pk;       // read above by these 4 lanes only, all of one wave
            float vf[16];
            cvt16(vr[i], vsc[i], vf);
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = fmaf(pk, vf[e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            *reinterpret_cast<f32x4_t*>(&red[slot][sub * 16 + 4 * e]) =
                f32x4_t{acc[4 * e], acc[4 * e + 1], acc[4 * e + 2], acc[4 * e + 3]};
        __syncthreads();
        if (tid < HD)
            chunk_tail<CHUNK>(sc[j], red, tid, m, nchunk == 1, out + (long)(b * S + j) * D + h * HD, po, pml);
        if (MS > 1) __syncthreads();                        // red is reused by the next query
    }
}

// attention_decode.hip's combine, copied: one block (64 threads = the 64 dims) per (row, h): out = sum_i w_i o_i /
// sum_i w_i l_i, w_i = exp2(m_i - M), chunk order
__global__ void __launch_bounds__(64) attn_decode_fp8_combine_kernel(const float* __restrict__ part,
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

struct DecArgs {
    const bf16_t* qkv;
    uint8_t *kcache, *vcache;
    float *kscale, *vscale;
    const int* lens;
    bf16_t* out;
    float* part;
    int B, S, H, Tmax;
    float scale;
};

template <int CHUNK, int MS>
void launch_decode(const DecArgs& a, hipStream_t st) {
    const int nchunk = (int)cdiv(a.Tmax, CHUNK);
    hipLaunchKernelGGL((attn_decode_fp8_kernel<CHUNK, MS>), dim3(a.B * a.H * nchunk), dim3(NTD), 0, st, a.qkv, a.kcache,
                       a.vcache, a.kscale, a.vscale, a.lens, a.out, a.part, a.S, a.H, a.Tmax, nchunk, a.scale);
    if (nchunk > 1)
        hipLaunchKernelGGL(attn_decode_fp8_combine_kernel, dim3(a.B * a.S * a.H), dim3(64), 0, st, (const float*)a.part,
                           a.out, nchunk);
}

template <int MS>
int decode_entry(const DecArgs& a, int chunk, hipStream_t st) {
    if (a.B < 1 || a.H < 1 || a.Tmax < 1 || a.S < 1 || a.S > MS || !a.qkv || !a.kcache || !a.vcache || !a.kscale ||
        !a.vscale || !a.lens || !a.out || !a.part)
        return (int)hipErrorInvalidValue;
    const long nblk = (long)a.B * a.H * cdiv(a.Tmax, chunk), n = nblk * a.S * (HD + 2);       // the partials, as bf16's
    if (n > 0x7fffffffL) return (int)hipErrorInvalidValue;
    if (chunk == 64)
        launch_decode<64, MS>(a, st);
    else if (chunk == 128)
        launch_decode<128, MS>(a, st);
    else if (chunk == 256)
        launch_decode<256, MS>(a, st);
    else
        return (int)hipErrorInvalidValue;
    PDNN_LAUNCH_RET;
}

// ------------------------------------------------------------------------------------------------ extend
constexpr int TILE = 64;        // queries per block
constexpr float RESC = 8.f;     // lazy-rescale threshold (log2 units), attention.hip's

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// The fragment helpers and the kernel body below are attention_extend.hip's (same tile image, same operand order, same
// arithmetic), copied so that its compiled kernel cannot change with this file; only the tile loader differs.
// [64][64] bf16 tile image, 128-byte rows, 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7)
__device__ __forceinline__ int toff(int row, int chunk) { return row * HD + ((chunk ^ ((row >> 1) & 7)) << 3); }

__device__ __forceinline__ bf16x8_t frag_rows(const bf16_t* img, int row0, int ks, int lane) {
    const int row = row0 + (lane & 15);
    return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(img + toff(row, ks * 4 + (lane >> 4))));
}

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

__device__ __forceinline__ bf16x8_t gfrag(const bf16_t* base, long ld, int ks, int lane) {
    const bf16_t* p = base + (long)(lane & 15) * ld + ks * 32 + 8 * (lane >> 4);
    return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(p));
}

// 64-key tile of the code rows of one (b, h): 256 threads x 2 LDS chunks = 8 codes and the row's scale each, held as
// codes while in flight and converted to the bf16 image when stored.  Row index clamped to Tmax - 1; a row past ``keep``
// becomes +0 (V: the block's last visible key; K: never, keep = INT_MAX)
struct CodeTile {
    uint2 r[2];
    float s[2];
    __device__ __forceinline__ void load(const uint8_t* rows, const float* scales, int k0, int Tmax, int keep, int tid) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int key = k0 + (tid >> 3) + 32 * i, ch = tid & 7;
            const long row = min(key, Tmax - 1);
            r[i] = *reinterpret_cast<const uint2*>(rows + row * HD + ch * 8);
            s[i] = scales[row];
            if (key > keep) {
                r[i] = make_uint2(0u, 0u);
                s[i] = 1.f;
            }
        }
    }
    __device__ __forceinline__ void store(bf16_t* img, int tid) const {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (tid >> 3) + 32 * i, ch = tid & 7;
            const bf16x2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[i].x, s[i], false);
            const bf16x2_t p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[i].x, s[i], true);
            const bf16x2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[i].y, s[i], false);
            const bf16x2_t p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[i].y, s[i], true);
            *reinterpret_cast<u32x4_t*>(img + toff(row, ch)) =
                u32x4_t{__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1),
                        __builtin_bit_cast(unsigned, p2), __builtin_bit_cast(unsigned, p3)};
        }
    }
};

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

__global__ void __launch_bounds__(NTD) attn_extend_fp8_kernel(const bf16_t* __restrict__ qkv,
                                                              const uint8_t* __restrict__ kcache,
                                                              const uint8_t* __restrict__ vcache,
                                                              const float* __restrict__ kscale,
                                                              const float* __restrict__ vscale,
                                                              const int* __restrict__ lens, bf16_t* __restrict__ out,
                                                              int Tq, int H, int Tmax, float scale) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[2][2][64 * HD];     // [buf][K|V]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
    const int nqt = Tq / TILE;
    const int t = blockIdx.x, HB = gridDim.x / nqt;         // 1-D grid of nqt x H x B blocks, late query tiles first
    const int r_ = t / HB, hb = t - r_ * HB;
    const int qt = nqt - 1 - r_, h = hb % H, b = hb / H;
    const int D = H * HD;
    const long ld = 3L * D;
    const int p0 = __builtin_amdgcn_readfirstlane(clamp_len(lens[b], Tmax));
    const uint8_t* Kc = kcache + ((long)b * H + h) * Tmax * HD;
    const uint8_t* Vc = vcache + ((long)b * H + h) * Tmax * HD;
    const float* Ks = kscale + ((long)b * H + h) * Tmax;
    const float* Vs = vscale + ((long)b * H + h) * Tmax;
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
    CodeTile ka, va, kn, vn;
    ka.load(Kc, Ks, 0, Tmax, NOKEEP, tid);
    va.load(Vc, Vs, 0, Tmax, blast, tid);
    ka.store(smem[0][0], tid);
    va.store(smem[0][1], tid);
    if (1 < nkb) {
        kn.load(Kc, Ks, 64, Tmax, NOKEEP, tid);
        vn.load(Vc, Vs, 64, Tmax, blast, tid);
    }
    __syncthreads();
    // tile kb is in LDS buffer cur = kb & 1; (hk, hv) hold tile kb + 1 in flight; (fk, fv) are free for kb + 2
    auto step = [&](const int kb, const int cur, CodeTile& hk, CodeTile& hv, CodeTile& fk, CodeTile& fv) {
        if (kb + 2 < nkb) {
            fk.load(Kc, Ks, (kb + 2) * 64, Tmax, NOKEEP, tid);
            fv.load(Vc, Vs, (kb + 2) * 64, Tmax, blast, tid);
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
}  // namespace

// prefill: qkv [B*T][3*H*64] bf16, T <= Tmax: K and V of every (b, t, h) quantised into slot t of kcache / vcache uint8
// [B][H][Tmax][64] and kscale / vscale fp32 [B][H][Tmax]; slots >= T are untouched
PDNN_API int pdnn_kv_cache_fill_fp8(const bf16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale, float* vscale,
                                    int B, int T, int H, int Tmax, hipStream_t st) {
    if (B < 1 || T < 1 || H < 1 || Tmax < 1 || T > Tmax || !qkv || !kcache || !vcache || !kscale || !vscale)
        return (int)hipErrorInvalidValue;
    const long total = (long)B * H * T * 8;
    hipLaunchKernelGGL(kv_cache_quant_kernel<false>, dim3(stream_grid(total, NTD)), dim3(NTD), 0, st, qkv, kcache, vcache,
                       kscale, vscale, (const int*)nullptr, T, H, Tmax, total);
    PDNN_LAUNCH_RET;
}

// qkv [B*Tq][3*H*64] bf16, lens int32 [B] (device): K and V of row b*Tq + j quantised into slot lens[b] + j (a slot >=
// Tmax is not stored); lens is not changed.  Tq a multiple of the extend tile, as pdnn_kv_cache_append.
PDNN_API int pdnn_kv_cache_append_fp8(const bf16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale, float* vscale,
                                      const int* lens, int B, int Tq, int H, int Tmax, hipStream_t st) {
    if (B < 1 || Tq < 1 || H < 1 || Tmax < 1 || Tq % TILE != 0 || !qkv || !kcache || !vcache || !kscale || !vscale || !lens)
        return (int)hipErrorInvalidValue;
    const long total = (long)B * H * Tq * 8;
    hipLaunchKernelGGL(kv_cache_quant_kernel<true>, dim3(stream_grid(total, NTD)), dim3(NTD), 0, st, qkv, kcache, vcache,
                       kscale, vscale, lens, Tq, H, Tmax, total);
    PDNN_LAUNCH_RET;
}

// qkv [B][3*H*64] bf16, the fp8 cache of the header, lens int32 [B] (device), out [B][H*64] bf16, part fp32
// [pdnn_attn_decode_ws].  chunk in {64, 128, 256}.
PDNN_API int pdnn_attn_decode_fp8(const bf16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale, float* vscale,
                                  const int* lens, bf16_t* out, float* part, int B, int H, int Tmax, int chunk,
                                  float scale, hipStream_t st) {
    return decode_entry<1>(DecArgs{qkv, kcache, vcache, kscale, vscale, lens, out, part, B, 1, H, Tmax, scale}, chunk, st);
}

// qkv [B*S][3*H*64] bf16, out [B*S][H*64] bf16, part fp32 [pdnn_attn_decode_multi_ws].  1 <= S <= 8.
PDNN_API int pdnn_attn_decode_multi_fp8(const bf16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale, float* vscale,
                                        const int* lens, bf16_t* out, float* part, int B, int S, int H, int Tmax,
                                        int chunk, float scale, hipStream_t st) {
    return decode_entry<MAXS>(DecArgs{qkv, kcache, vcache, kscale, vscale, lens, out, part, B, S, H, Tmax, scale}, chunk,
                              st);
}

// after pdnn_kv_cache_append_fp8 of the same qkv on the same stream: out [B*Tq][H*64] bf16, query row b*Tq + j at
// position lens[b] + j over the cache keys 0 .. lens[b] + j
PDNN_API int pdnn_attn_extend_fp8(const bf16_t* qkv, const uint8_t* kcache, const uint8_t* vcache, const float* kscale,
                                  const float* vscale, const int* lens, bf16_t* out, int B, int Tq, int H, int Tmax,
                                  float scale, hipStream_t st) {
    if (B < 1 || Tq < 1 || H < 1 || Tmax < 1 || Tq % TILE != 0 || !qkv || !kcache || !vcache || !kscale || !vscale ||
        !lens || !out)
        return (int)hipErrorInvalidValue;
    const long nblk = (long)B * H * (Tq / TILE);
    if (nblk > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(attn_extend_fp8_kernel, dim3((unsigned)nblk), dim3(NTD), 0, st, qkv, kcache, vcache, kscale, vscale,
                       lens, out, Tq, H, Tmax, scale);
    PDNN_LAUNCH_RET;
}
