"""The bookkeeping of a speculative decode step in plain torch: ``prepare_reference`` and ``accept_reference`` implement
the definitions in the header of csrc/kernels/speculate.hip line for line, run on any device, and are what
``GPT2.generate(speculate=S)`` uses on the CPU.  They are the reference of the two kernels (exact integers, exact u).

State: ``out`` int64 [B][P + N] (prompts in columns < P, new tokens from column P), ``prompt_len``, ``ntok`` (tokens
emitted) and ``lens`` (tokens cached) int32 [B], ``finished`` uint8 [B]."""
import torch

from .sampling import uniform


def history(out, P, prompt_len, ntok, b):
    """h of row b as a list: the prompt, then the tokens emitted so far"""
    pl, nt = int(prompt_len[b]), int(ntok[b])
    return out[b, :pl].tolist() + out[b, P:P + nt].tolist()


def ngram_drafts(h, ngram, count):
    """prompt lookup: ``count`` drafts continuing the latest earlier occurrence of the longest matching suffix of h"""
    Lh = len(h)
    for n in range(min(int(ngram), Lh - 1), 0, -1):
        for s in range(Lh - n - 1, -1, -1):
            if h[s:s + n] == h[Lh - n:]:
                return [h[min(s + n + i, Lh - 1)] for i in range(count)]
    return [h[-1]] * count


def prepare_reference(out, P, N, prompt_len, ntok, lens, seed, S, guess=None, ngram=3):
    """-> (tok_in int64 [B*S], pos int32 [B*S], u fp32 [B*S]): row b*S is the last emitted token of row b, rows b*S+1..
    its S-1 drafts (``guess`` int64 [B][N]: d_i = guess[b, min(ntok[b] + i, N-1)]; else the n-gram lookup); pos = lens[b]
    + j; u = the draw of (seed, step = ntok[b] + j, stream = b)."""
    B = out.shape[0]
    tok, pos, u = [], [], []
    for b in range(B):
        h = history(out, P, prompt_len, ntok, b)
        nt = int(ntok[b])
        if guess is not None:
            d = [int(guess[b, min(nt + i, N - 1)]) for i in range(S - 1)]
        else:
            d = ngram_drafts(h, ngram, S - 1)
        tok += [h[-1]] + d
        pos += [int(lens[b]) + j for j in range(S)]
        u += [uniform(seed, nt + j, b) for j in range(S)]
    dev = out.device
    return (torch.tensor(tok, dtype=torch.int64, device=dev), torch.tensor(pos, dtype=torch.int32, device=dev),
            torch.tensor(u, dtype=torch.float32, device=dev))


def accept_reference(tok_in, t, out, P, N, ntok, lens, finished, eos_token, stats, S):
    """Compare the drafts in ``tok_in`` with the drawn tokens ``t`` (both int64 [B*S]) and advance ``out``, ``ntok``,
    ``lens``, ``finished`` (None without an eos) and ``stats`` int64 [S+1] in place.  Returns done: every row complete."""
    B = out.shape[0]
    ti, tt = tok_in.tolist(), t.tolist()
    done = True
    for b in range(B):
        nt = int(ntok[b])
        if nt >= N:
            continue
        fin = eos_token is not None and bool(finished[b])
        e = 0
        if not fin:
            for i in range(S):
                if e >= N - nt:
                    break
                tok = tt[b * S + i]
                out[b, P + nt + e] = tok
                e += 1
                if eos_token is not None and tok == int(eos_token):
                    fin = True
                    break
                if i + 1 < S and ti[b * S + 1 + i] != tok:
                    break
        lens[b] += e
        nt += e
        if fin:
            out[b, P + nt:P + N] = int(eos_token)
            nt = N
            finished[b] = 1
        ntok[b] = nt
        stats[e] += 1
        done = done and nt >= N
    return done
