// The dropout generator: one stateless, counter-based function, used by every kernel that drops (the flash-attention
// DROP variants in attention.hip, the row kernels and the mask exports in dropout.hip).  No mask is ever stored: the
// forward and the backward derive the same bits from the same (seed, step, site, coordinates).
// tests/dropout_ref.py (numpy) and ops/transformer.py dropout_keep_reference (torch) re-implement it line for line.
//
// Definition (all arithmetic unsigned and wrapping, in the stated width).
//   state    int64[2] in device memory: (seed, step).  A kernel reads it from memory, so a captured step sees the values
//            of the replay, not of the capture.
//   site     uint32: which dropout of the model.  layer * 4 + 0 attention probabilities, + 1 attention-branch residual,
//            + 2 MLP-branch residual; 0x7fffffff the embedding; 0x7ffffffe the token draw of sample.hip (stream = row).
//   stream   uint32: b * H + h for attention, 0 for a row op.
//   key      z = mix64(seed + 0x9E3779B97F4A7C15 * (step + 1));  z = mix64(z ^ (site << 32 | stream));
//            k0 = low 32 bits of z, k1 = high 32 bits;  mix64 is the splitmix64 finaliser
//            (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31).
//            Once per block (uniform: scalar registers), never per element.
//   granule  4 consecutive elements along the fastest coordinate share one 32-bit word:
//              attention (q, k):   idx = q * (T / 4) + (k >> 2),    element j = k & 3      (T % 4 == 0, T <= 65536)
//              rows (row, col):    idx = row * (D / 4) + (col >> 2), element j = col & 3   (D % 4 == 0, R * D / 4 <= 2^32)
//            so idx < 2^32 is a bijection of the granule's coordinates.
//   word     x = idx + k0;  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x += k1;  x *= 0x846ca68b;  x ^= x >> 16
//            (the "lowbias32" integer hash, a bijection of x, with the second key word added between its two
//            multiplies: two streams are not shifted copies of each other).
//   keep     element j is kept iff byte j of the word, (word >> 8 j) & 255, is >= thr.
//   thr      floor(256 p + 1/2) clamped to 255, for p in [0, 1): the probability is quantised to 8 bits,
//            p_eff = thr / 256 (pdnn_dropout_p_eff), and every consumer scales by 1 / (1 - p_eff) = 256 / (256 - thr).
//            p = 0.1 gives thr 26, p_eff = 0.1015625.  Anything outside [0, 1) (NaN included) is refused before launch.
//
// Why this granule.  The forward and the dQ kernel hold, per lane, the 4 consecutive keys 16 kf + 4 g + r of one query:
// exactly one word, all four bytes used.  The dK / dV kernel holds 4 consecutive queries of one key: four words, one
// byte of each used.  A word is 9 VALU instructions, two of them v_mul_lo_u32 (one add of the tile-relative index, the
// add of k1, two shift-xor pairs and a last one); an element is 2 to 3 more (byte extract, compare, select).
// Predicted cost per lane and 64-key (64-query) tile:
//   forward  (32 elements):     8 words =  72 + 32 selects ~ 100 VALU on top of ~ 200 (the tile's 32 exp2 / fma / max / cvt)
//   dQ       (16 NF elements):  4 NF words = 36 NF + 16 NF selects and scale multiplies ~ 70 NF
//   dK / dV  (16 NF elements): 16 NF words = 144 NF + 32 NF selects ~ 175 NF: about as much again as the tile's own VALU
// A 4 x 4-block granule (Philox4x32: 128 bits per block) would serve dK / dV from one call but costs the forward a whole
// Philox (ten rounds of two 32 x 32 -> 64 multiplies) for four bytes; profiles/attention_dropout.txt has the measurement
// that decides whether this choice stands (p = 0.1, B8 T1024 H12: forward + 24 %, backward + 28 % with dK / dV on its
// 16-key kernel; the 32-key dK / dV kernel with DROP fell to one wave / SIMD and is not built).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pdrop {
constexpr uint32_t SITE_EMBD = 0x7fffffffu;
constexpr uint32_t SITE_SAMPLE = 0x7ffffffeu;

struct Key {
    uint32_t k0, k1;
};

// what a launcher hands a kernel: the state pointer and the quantised probability
struct Arg {
    const long long* state;     // device int64[2]: seed, step
    uint32_t site;
    uint32_t thr;               // keep iff byte >= thr
    float scale;                // 256 / (256 - thr)
};

// p in [0, 1) -> thr; false for anything else
inline bool threshold(float p, uint32_t* thr) {
    if (!(p >= 0.f && p < 1.f)) return false;
    const uint32_t t = (uint32_t)((double)p * 256.0 + 0.5);
    *thr = t > 255u ? 255u : t;
    return true;
}
inline float scale_of(uint32_t thr) { return 256.f / (float)(256u - thr); }

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__device__ __forceinline__ Key stream_key(const long long* state, uint32_t site, uint32_t stream) {
    const uint64_t seed = (uint64_t)state[0], step = (uint64_t)state[1];
    uint64_t z = mix64(seed + 0x9E3779B97F4A7C15ull * (step + 1));
    z = mix64(z ^ (((uint64_t)site << 32) | stream));
    return Key{(uint32_t)z, (uint32_t)(z >> 32)};
}

// the word of granule idx, from x = idx + k0
__device__ __forceinline__ uint32_t word_x(uint32_t x, uint32_t k1) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x += k1;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t word(const Key& k, uint32_t idx) { return word_x(idx + k.k0, k.k1); }
__device__ __forceinline__ bool keep(uint32_t w, int j, uint32_t thr) { return ((w >> (8 * j)) & 255u) >= thr; }
}  // namespace pdrop
