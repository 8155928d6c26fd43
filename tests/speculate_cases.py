"""Hand-written cases of the speculative step's bookkeeping (csrc/kernels/speculate.hip, ops/speculate.py), shared by
tests/test_speculate_ref_cpu.py (the torch references) and tests/test_speculate_gpu.py (the kernels).  Every expected
value below was worked out by hand from the definition in the kernel file's header, not produced by either
implementation."""
import torch

I32, I64 = torch.int32, torch.int64
PAD = 99            # padding between a short prompt and the new tokens: never part of a history


def _row(prompt, P, new, N):
    return prompt + [PAD] * (P - len(prompt)) + new + [0] * (N - len(new))


# name -> (P, N, S, ngram, prompt, new tokens so far, expected tok_in)
PREPARE_NGRAM = {
    # suffix [1, 2, 3] occurs at s = 0: the drafts continue it with 4, 5, 1
    "match_n3": (8, 6, 4, 3, [1, 2, 3, 4, 5, 1, 2], [3], [3, 4, 5, 1]),
    # [6, 5, 3] and [5, 3] occur nowhere earlier; [3] occurs at s = 3: drafts h[4], h[5], h[6]
    "fallback_n1": (5, 6, 4, 3, [7, 8, 9, 3, 6], [5, 3], [3, 6, 5, 3]),
    "no_match": (4, 6, 4, 3, [1, 2, 3, 4], [], [4, 4, 4, 4]),
    # [1, 2] at s = 0 continues 9, 1, 2 and then runs off the end of the history: the last token repeats
    "off_the_end": (3, 8, 6, 3, [1, 2, 9], [1, 2], [2, 9, 1, 2, 2, 2]),
    # [1, 2] occurs at s = 0 and s = 3: the later one wins, drafts 8, 1, 2
    "largest_s": (6, 8, 4, 3, [1, 2, 7, 1, 2, 8], [1, 2], [2, 8, 1, 2]),
    # prompt of 3 in 6 columns: h = [1, 2, 3, 1, 2], [1, 2] at s = 0 -> 3, 1, 2 (a lookup into the padding would give 99)
    "ragged_padding": (6, 6, 4, 3, [1, 2, 3], [1, 2], [2, 3, 1, 2]),
    # ngram = 1 on a history of one token: n = min(1, 0) = 0, nothing to look up
    "one_token": (1, 4, 3, 1, [5], [], [5, 5, 5]),
    # ngram larger than the history: n starts at Lh - 1 = 2, [4, 4] at s = 0 -> h[2], h[2]
    "long_ngram": (2, 4, 3, 7, [4, 4], [4], [4, 4, 4]),
}


def prepare_ngram_case(name, device="cpu"):
    """-> (kwargs of prepare_reference / the state tensors, expected tok_in, pos, ntok)"""
    P, N, S, ngram, prompt, new, want = PREPARE_NGRAM[name]
    out = torch.tensor([_row(prompt, P, new, N)], dtype=I64, device=device)
    pl = torch.tensor([len(prompt)], dtype=I32, device=device)
    ntok = torch.tensor([len(new)], dtype=I32, device=device)
    lens = torch.tensor([len(prompt) + len(new) - 1], dtype=I32, device=device)
    return dict(out=out, P=P, N=N, prompt_len=pl, ntok=ntok, lens=lens, S=S, ngram=ngram), want


def prepare_table_case(device="cpu"):
    """B = 2, S = 4, N = 5: row 0 has emitted 2 tokens, row 1 has emitted 4 (its table index saturates at N - 1)"""
    P, N, S = 3, 5, 4
    out = torch.tensor([_row([1, 2, 3], P, [10, 11], N), _row([4], P, [20, 21, 22, 23], N)], dtype=I64, device=device)
    guess = torch.tensor([[50, 51, 52, 53, 54], [60, 61, 62, 63, 64]], dtype=I64, device=device)
    kw = dict(out=out, P=P, N=N, prompt_len=torch.tensor([3, 1], dtype=I32, device=device),
              ntok=torch.tensor([2, 4], dtype=I32, device=device), lens=torch.tensor([4, 4], dtype=I32, device=device),
              S=S, guess=guess)
    return kw, [11, 52, 53, 54, 23, 64, 64, 64], [4, 5, 6, 7, 4, 5, 6, 7]


def accept_case(device="cpu"):
    """B = 8, S = 4, P = 2, N = 10, eos = 7.  Rows:
      0  a = 0: the first draft (6) is not the drawn token (9): emits [9]
      1  a = S - 1: every draft is right: emits [6, 8, 3, 4]
      2  a mismatch in the middle: drafts 6, 8 right, draft 3 drawn as 1: emits [6, 8, 1]
      3  truncation: 8 tokens emitted already, two columns left, all drafts right: emits [6, 8]
      4  eos inside an accepted run: the second drawn token is 7: emits [6, 7], the rest of the row becomes 7
      5  finished by the first draw (token 0 was eos): emits nothing, the rest of the row becomes 7
      6  complete: nothing changes
      7  a = 0 with the eos drawn at once: emits [7], then eos"""
    P, N, S, eos = 2, 10, 4, 7
    new = [[5], [5], [5], [1, 2, 3, 4, 1, 2, 3, 5], [5], [7], [1, 2, 3, 4, 5, 6, 1, 2, 3, 4], [5]]
    tok_in = [[5, 6, 8, 3]] * 5 + [[7, 6, 8, 3], [4, 6, 8, 3], [5, 6, 8, 3]]
    t = [[9, 1, 1, 1], [6, 8, 3, 4], [6, 8, 1, 2], [6, 8, 3, 4], [6, 7, 3, 4], [1, 2, 3, 4], [6, 8, 3, 4], [7, 8, 3, 4]]
    state = dict(
        tok_in=torch.tensor(tok_in, dtype=I64, device=device).reshape(-1),
        t=torch.tensor(t, dtype=I64, device=device).reshape(-1),
        out=torch.tensor([_row([1, 2], P, n, N) for n in new], dtype=I64, device=device),
        ntok=torch.tensor([len(n) for n in new], dtype=I32, device=device),
        lens=torch.tensor([1 + len(n) for n in new], dtype=I32, device=device),
        finished=torch.tensor([0, 0, 0, 0, 0, 1, 0, 0], dtype=torch.uint8, device=device),
        stats=torch.tensor([3, 0, 0, 0, 1], dtype=I64, device=device))
    after = [[5, 9], [5, 6, 8, 3, 4], [5, 6, 8, 1], [1, 2, 3, 4, 1, 2, 3, 5, 6, 8], [5, 6] + [7] * 8, [7] * 10,
             [1, 2, 3, 4, 5, 6, 1, 2, 3, 4], [5] + [7] * 9]
    want = dict(out=[_row([1, 2], P, n, N) for n in after], ntok=[2, 5, 4, 10, 10, 10, 10, 10],
                lens=[3, 6, 5, 11, 4, 2, 11, 3], finished=[0, 0, 0, 0, 1, 1, 0, 1],
                stats=[3 + 1, 0 + 2, 0 + 2, 0 + 1, 1 + 1], done=False)
    return dict(P=P, N=N, S=S, eos_token=eos), state, want


def accept_done_case(device="cpu"):
    """B = 2, S = 2, P = 1, N = 3, no eos: row 0 emits its last token, row 1 is complete: done"""
    P, N, S = 1, 3, 2
    state = dict(tok_in=torch.tensor([3, 4, 9, 9], dtype=I64, device=device),
                 t=torch.tensor([4, 5, 1, 1], dtype=I64, device=device),
                 out=torch.tensor([[1, 2, 3, 0], [1, 7, 8, 9]], dtype=I64, device=device),
                 ntok=torch.tensor([2, 3], dtype=I32, device=device), lens=torch.tensor([2, 3], dtype=I32, device=device),
                 finished=None, stats=torch.zeros(S + 1, dtype=I64, device=device))
    want = dict(out=[[1, 2, 3, 4], [1, 7, 8, 9]], ntok=[3, 3], lens=[3, 3], finished=None, stats=[0, 1, 0], done=True)
    return dict(P=P, N=N, S=S, eos_token=None), state, want
