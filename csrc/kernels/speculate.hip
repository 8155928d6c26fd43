// The two bookkeeping kernels of a speculative decode step (GPT2.generate(speculate=S)): pdnn_spec_prepare builds the S
// input rows of every sequence from the state on the device, pdnn_spec_accept compares the drafts with the tokens the
// verify forward drew and advances the state.  ops/speculate.py (prepare_reference, accept_reference) is the same
// definition in torch.  Plain C++, vector stores, no atomics; B <= 8 sequences, 2 <= S <= 8 rows each (S = 1 works too).
//
// State.  out int64 [B][ld]: columns 0..P-1 the prompts (row b's is out[b, :prompt_len[b]], the rest padding), columns
// P..P+N-1 the new tokens.  ntok int32 [B]: tokens row b has emitted (>= 1: the first is drawn from the prefill logits).
// lens int32 [B]: tokens in the key/value cache, prompt_len[b] + ntok[b] - 1 while the row is incomplete.  The history
// of row b is h = out[b, :prompt_len[b]] ++ out[b, P : P + ntok[b]], of length Lh.
//
// pdnn_spec_prepare (one block per row) writes, for j = 0..S-1:
//   tok_in[b*S + j]  h[Lh-1] for j = 0 (the last emitted token), draft d_{j-1} otherwise
//   pos[b*S + j]     lens[b] + j
//   u[b*S + j]       the uniform of sample.hip for (seed, step = ntok[b] + j, stream = b): word 0 of
//                    pdrop::stream_key(.., SITE_SAMPLE, b), >> 8, times 2^-24
// Drafts, n-gram (prompt lookup, guess == null): for n = min(ngram, Lh-1) down to 1, the largest s in [0, Lh-n-1] with
// h[s : s+n] == h[Lh-n : Lh]; the first n with a match wins and d_i = h[min(s+n+i, Lh-1)]; no match: d_i = h[Lh-1].
// Drafts, table (guess int64 [B][N]): d_i = guess[b, min(ntok[b] + i, N-1)].
// prompt_len is clamped into [1, P] and ntok into [0, N] before either becomes an address.
//
// pdnn_spec_accept (one block), after the verify forward has drawn t int64 [B*S]: for a row with ntok[b] < N, a is the
// largest value with tok_in[b*S+1+i] == t[b*S+i] for all i < a; the row emits t[b*S + 0..a], cut to the N - ntok[b]
// columns left and after the first eos, into out[b, P + ntok[b] ..]; ntok[b] and lens[b] advance by the number e emitted.
// If an emitted token is eos, or finished[b] was set on entry (then e = 0), the remaining columns become eos, ntok[b] = N
// and finished[b] = 1.  A complete row (ntok[b] >= N) emits nothing and its lens does not move.  done[0] = every row is
// complete; stats[e] += 1 for every row that was incomplete on entry.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): spec_prepare_kernel 14 VGPRs, 16 bytes LDS;
// spec_accept_kernel 16 VGPRs, 96 bytes LDS; scratch 0 in both.
#include "common.h"
#include "dropout_rng.h"

namespace {
constexpr int PNT = 256;
constexpr int MAXB = 8, MAXS = 8;

// element i of row b's history: the prompt, then the new tokens
__device__ __forceinline__ long long hist_at(const long long* row, int P, int pl, int i) {
    return i < pl ? row[i] : row[P + i - pl];
}

__global__ void __launch_bounds__(PNT) spec_prepare_kernel(const long long* __restrict__ out, int ld, int P, int N,
                                                           const int* __restrict__ prompt_len,
                                                           const int* __restrict__ ntok, const int* __restrict__ lens,
                                                           long long seed, const long long* __restrict__ guess, int ngram,
                                                           int S, long long* __restrict__ tok_in, int* __restrict__ pos,
                                                           float* __restrict__ u) {
    __shared__ int wbest[PNT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long* row = out + (long)b * ld;
    const int pl = min(max(prompt_len[b], 1), P), nt = min(max(ntok[b], 0), N), Lh = pl + nt;
    if (tid < S) {
        pos[b * S + tid] = lens[b] + tid;
        const long long st[2] = {seed, (long long)nt + tid};
        const pdrop::Key k = pdrop::stream_key(st, pdrop::SITE_SAMPLE, (uint32_t)b);
        u[b * S + tid] = (float)(pdrop::word(k, 0) >> 8) * 0x1p-24f;
    }
    const long long last = hist_at(row, P, pl, Lh - 1);
    if (guess) {
        if (tid < S) tok_in[b * S + tid] = tid == 0 ? last : guess[(long)b * N + min(nt + tid - 1, N - 1)];
        return;
    }
    int best = -1, bn = 0;
    for (int n = min(ngram, Lh - 1); n >= 1; --n) {         // block-uniform loop
        int cand = -1;
        for (int s = tid; s <= Lh - n - 1; s += PNT) {      // ascending: the last hit of a thread is its largest
            bool eq = true;
            for (int e = 0; e < n; ++e)
                if (hist_at(row, P, pl, s + e) != hist_at(row, P, pl, Lh - n + e)) {
                    eq = false;
                    break;
                }
            if (eq) cand = s;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) cand = max(cand, __shfl_xor(cand, m));
        if ((tid & 63) == 0) wbest[tid >> 6] = cand;
        __syncthreads();
        best = max(max(wbest[0], wbest[1]), max(wbest[2], wbest[3]));
        __syncthreads();
        if (best >= 0) {
            bn = n;
            break;
        }
    }
    if (tid < S)
        tok_in[b * S + tid] = (tid == 0 || best < 0) ? last : hist_at(row, P, pl, min(best + bn + tid - 1, Lh - 1));
}

__global__ void __launch_bounds__(PNT) spec_accept_kernel(const long long* __restrict__ tok_in,
                                                          const long long* __restrict__ t, long long* __restrict__ out,
                                                          int ld, int P, int N, int* __restrict__ ntok,
                                                          int* __restrict__ lens, unsigned char* __restrict__ finished,
                                                          long long eos, int* __restrict__ done,
                                                          long long* __restrict__ stats, int B, int S) {
    __shared__ int fill_from[MAXB], emitted[MAXB], complete[MAXB];
    const int tid = threadIdx.x;
    if (tid < B) {                                          // one thread walks one row: at most S tokens
        const int b = tid;
        long long* row = out + (long)b * ld + P;
        int nt = min(max(ntok[b], 0), N), e = -1, fill = N;
        if (nt < N) {
            bool fin = eos >= 0 && finished[b] != 0;
            e = 0;
            if (!fin) {
                const int room = N - nt;
                for (int i = 0; i < S && e < room; ++i) {
                    const long long tok = t[b * S + i];
                    row[nt + e] = tok;
                    ++e;
                    if (eos >= 0 && tok == eos) {
                        fin = true;
                        break;
                    }
                    if (i + 1 < S && tok_in[b * S + 1 + i] != tok) break;
                }
            }
            lens[b] += e;
            nt += e;
            if (fin) {
                fill = nt;
                nt = N;
                finished[b] = 1;
            }
            ntok[b] = nt;
        }
        fill_from[b] = fill;
        emitted[b] = e;
        complete[b] = nt >= N;
    }
    __syncthreads();
    for (int b = 0; b < B; ++b)
        for (int col = fill_from[b] + tid; col < N; col += PNT) out[(long)b * ld + P + col] = eos;
    if (tid == 0) {
        int all = 1;
        for (int b = 0; b < B; ++b) {
            all &= complete[b];
            if (emitted[b] >= 0) stats[emitted[b]] += 1;
        }
        done[0] = all;
    }
}
}  // namespace

// out int64 [B][ld] (ld >= P + N), prompt_len / ntok / lens int32 [B], guess int64 [B][N] or null (n-gram drafts),
// tok_in int64 [B*S], pos int32 [B*S], u fp32 [B*S].  1 <= B <= 8, 1 <= S <= 8, P, N, ngram >= 1.
PDNN_API int pdnn_spec_prepare(const long long* out, int ld, int P, int N, const int* prompt_len, const int* ntok,
                               const int* lens, long long seed, const long long* guess, int ngram, int B, int S,
                               long long* tok_in, int* pos, float* u, hipStream_t st) {
    if (B < 1 || B > MAXB || S < 1 || S > MAXS || P < 1 || N < 1 || ngram < 1 || (long)P + N > ld || !out ||
        !prompt_len || !ntok || !lens || !tok_in || !pos || !u)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_prepare_kernel, dim3(B), dim3(PNT), 0, st, out, ld, P, N, prompt_len, ntok, lens, seed, guess,
                       ngram, S, tok_in, pos, u);
    PDNN_LAUNCH_RET;
}

// tok_in, t int64 [B*S]; out, ntok, lens as above; finished uint8 [B] (required when eos >= 0; eos < 0: no eos);
// done int32 [1]; stats int64 [S+1].
PDNN_API int pdnn_spec_accept(const long long* tok_in, const long long* t, long long* out, int ld, int P, int N, int* ntok,
                              int* lens, unsigned char* finished, long long eos, int* done, long long* stats, int B, int S,
                              hipStream_t st) {
    if (B < 1 || B > MAXB || S < 1 || S > MAXS || P < 1 || N < 1 || (long)P + N > ld || !tok_in || !t || !out || !ntok ||
        !lens || !done || !stats || (eos >= 0 && !finished))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(PNT), 0, st, tok_in, t, out, ld, P, N, ntok, lens, finished, eos,
                       done, stats, B, S);
    PDNN_LAUNCH_RET;
}
