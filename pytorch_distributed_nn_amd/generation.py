"""GPT-2 generation behind ``GPT2.generate`` (its docstring is the contract): one check of the arguments, one GPU
:class:`Engine` (``rows`` is the one copy of the decode forward), its CPU :class:`Reference`, one :class:`Replay` helper,
and per sampler a short unit around ``Engine.rows`` with its driver.  ``resume=True`` ingests through ``Engine.extend``
behind a kept cache instead of ``prefill``; :class:`Session` keeps the accounting of a conversation over several such
calls.  Kernels are called as ``K.name`` / ``BL.name``."""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn.functional as F

from . import tuning
from .ops import functional as OF
from .ops import kernels as K
from .ops import linear as BL
from .ops import transformer as TX
from .ops.sampling import sample_reference
from .ops.speculate import accept_reference, prepare_reference


def sample(logits, temperature, top_k, generator, top_p=None):
    """fp32 logits [B][V] -> token ids [B]: argmax for temperature 0 or top_k 1, else temperature, top-k, top-p (a
    sort: the smallest set of the most probable tokens whose mass reaches top_p), multinomial"""
    if temperature == 0 or top_k == 1:
        return logits.argmax(-1)
    lg = logits / temperature
    if top_k is not None:
        kth = torch.topk(lg, min(int(top_k), lg.shape[-1]), dim=-1).values[:, -1:]
        lg = lg.masked_fill(lg < kth, float("-inf"))
    if top_p is not None and top_p < 1:
        sl, si = torch.sort(lg, dim=-1, descending=True)
        sp = torch.softmax(sl, -1)
        drop = sp.cumsum(-1) - sp >= top_p                     # the mass before a token already reaches top_p
        lg = lg.masked_fill(torch.zeros_like(drop).scatter_(-1, si, drop), float("-inf"))
    return torch.multinomial(torch.softmax(lg, -1), 1, generator=generator).squeeze(1)


# one checked call: N = max_new_tokens, pl = the B prompt lengths, draw = dict(temperature, top_k, top_p), seed masked to
# 63 bits (sampler="device", else None), S = speculate or None, guess = the draft table or None (n-gram drafts)
Request = namedtuple("Request", "B P N pl draw eos generator seed S guess ngram graph return_logits return_stats cache "
                     "resume", defaults=(False,))


def check_args(c, idx, max_new_tokens, *, temperature, top_k, eos_token, prompt_lens, generator, graph,
               return_logits, cache, top_p, sampler, seed, speculate, draft, ngram, return_stats, resume=False):
    """``generate``'s arguments and the model's config ``c`` -> :class:`Request`, or the first refusal in this order"""
    if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError(f"generate: idx must be [B][P] with B, P >= 1, got {tuple(idx.shape)}")
    B, P = idx.shape
    max_new_tokens = int(max_new_tokens)
    if max_new_tokens < 0:
        raise ValueError(f"generate: max_new_tokens must be >= 0, got {max_new_tokens}")
    if prompt_lens is None:
        pl = [P] * B
    else:
        pl = [int(v) for v in (prompt_lens.tolist() if torch.is_tensor(prompt_lens) else prompt_lens)]
        if len(pl) != B or min(pl) < 1 or max(pl) > P:
            raise ValueError(f"generate: prompt_lens must be {B} lengths in [1, {P}], got {pl}")
    if max(pl) + max_new_tokens > c.block_size:
        raise ValueError(f"generate: prompt length {max(pl)} + max_new_tokens {max_new_tokens} > block size "
                         f"{c.block_size}")
    if temperature < 0 or (top_k is not None and int(top_k) < 1):
        raise ValueError(f"generate: temperature must be >= 0 and top_k >= 1, got {temperature!r}, {top_k!r}")
    if top_p is not None and not float(top_p) > 0:
        raise ValueError(f"generate: top_p must be > 0, got {top_p!r}")
    if sampler not in ("torch", "device"):
        raise ValueError(f"generate: sampler must be 'torch' or 'device', got {sampler!r}")
    if sampler == "device" and (generator is not None or seed is None):
        raise ValueError("generate: sampler='device' draws from seed: pass seed, and no generator")
    S = guess = None
    if speculate is not None:
        S = int(speculate)
        if not 2 <= S <= 8:
            raise ValueError(f"generate: speculate must be in [2, 8], got {speculate!r}")
        if sampler != "device":
            raise ValueError("generate: speculate verifies drafts with the counter-based draw: pass sampler='device' "
                             "and a seed")
        if return_logits:
            raise ValueError("generate: return_logits is not available with speculate")
        if torch.is_tensor(draft):
            if draft.dtype != torch.int64 or draft.shape != (B, max_new_tokens):
                raise ValueError(f"generate: a draft table must be int64 [{B}][{max_new_tokens}], got {draft.dtype} "
                                 f"{tuple(draft.shape)}")
            guess = draft
        elif draft != "ngram":
            raise ValueError(f"generate: draft must be 'ngram' or an int64 [B][max_new_tokens] tensor, got {draft!r}")
        if not isinstance(ngram, int) or ngram < 1:
            raise ValueError(f"generate: ngram must be an int >= 1, got {ngram!r}")
        if idx.is_cuda and (not tuning.get("decode_skinny") or B > K.SKINNY_MAX_M or B * S > K.SKINNY_ROWS):
            raise ValueError(f"generate: speculate on the GPU needs tuning decode_skinny on, B <= {K.SKINNY_MAX_M} "
                             f"and B * S <= {K.SKINNY_ROWS} (the verify rows must get the bits of the plain step's "
                             f"skinny GEMM); got decode_skinny = {tuning.get('decode_skinny')!r}, B = {B}, S = {S}")
    elif return_stats:
        raise ValueError("generate: return_stats needs speculate")
    if idx.is_cuda:
        TX.need_fused_kernels(c.n_embd, c.n_head)
    if resume:
        check_resume(c, idx, B, pl, max_new_tokens, S, cache)
    return Request(B, P, max_new_tokens, pl, dict(temperature=float(temperature), top_k=top_k, top_p=top_p), eos_token,
                   generator, int(seed) & ((1 << 63) - 1) if sampler == "device" else None, S, guess, ngram, graph,
                   return_logits, return_stats, cache, bool(resume))


def check_resume(c, idx, B, pl, N, S, cache):
    """The refusals of ``resume=True``, after every other one.  The last reads cache.lens to the host, the call's one
    read-back before its first launch: every row must fit lens[b] + prompt_lens[b] + max_new_tokens (+ S)."""
    if cache is None or getattr(cache, "B", None) != B:
        raise ValueError(f"generate: resume=True continues a kept cache: pass cache=, an ops.transformer.KVCache of B = "
                         f"{B}, got {'none' if cache is None else f'one of B = {cache.B}'}")
    if not idx.is_cuda:
        raise ValueError("generate: resume=True runs on the GPU only (the CPU path keeps no cache between calls); "
                         "generation.Session (GPT2.session) holds a conversation on either device")
    if cache.k.device != idx.device or (S or 1) > cache.S:
        raise ValueError(f"generate: resume=True with a cache of S = {cache.S} on {cache.k.device}, need S >= {S or 1} on "
                         f"{idx.device}")
    room, extra = min(c.block_size, cache.Tmax), N + (S or 0)
    for b, (have, new) in enumerate(zip(cache.lens.tolist(), pl)):
        if have < 0 or have + new + extra > room:
            raise ValueError(f"generate: resume=True, row {b}: {have} cached + {new} new + {extra} to generate > "
                             f"{room} = min(block size, cache Tmax)")


class Replay:
    """``unit`` once per call: the first call runs it eagerly (the warm-up; with ``graph`` false every call does), the
    next one captures it with torch.cuda.graph, which does not execute it, and replays; every later call replays."""

    def __init__(self, unit, graph):
        self.unit, self.graph, self.warm, self.g = unit, graph, False, None

    def __call__(self):
        if not (self.graph and self.warm):
            self.warm = True
            return self.unit()
        if self.g is None:
            self.g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g):
                self.unit()
        self.g.replay()


class Engine:
    """One call's GPU model: the cache (``cache`` if it fits, reset; else a new one), bf16 shadows, block parameters"""

    def __init__(self, model, B, P, N, S=1, cache=None, resume=False):
        self.config, tr = model.config, model.transformer
        dev = tr.wte.weight.device
        Tneed = model.kv_cache_len(P, N + (S if S > 1 else 0))       # rejected drafts occupy slots past the accepted length
        if resume:                                      # check_resume has held the kept cache against this call
            pass
        elif cache is None:
            cache = TX.KVCache(model, B, Tneed, dev, S=S)
        elif cache.B != B or cache.Tmax < Tneed or cache.k.device != dev or cache.S < S:
            raise ValueError(f"generate: cache of B = {cache.B}, Tmax = {cache.Tmax}, S = {cache.S} on {cache.k.device} does "
                             f"not fit B = {B}, Tmax >= {Tneed}, S >= {S} on {dev}")
        if not resume:
            cache.reset()
        self.B, self.cache = B, cache
        self.wte_k, self.wpe_k = OF.weight_bf16(tr.wte.weight), OF.weight_bf16(tr.wpe.weight)
        self.blocks = [blk.fused_params() for blk in tr.h]
        self.lnw, self.lnb = tr.ln_f.weight, tr.ln_f.bias

    def prefill(self, idx, pl_dev):
        """idx int64 [B][P], pl_dev int32 [B] -> bf16 logits [B][V] at each prompt's last position; cache.lens = pl_dev"""
        c, cache = self.config, self.cache
        B, P = idx.shape
        Tp = (P + 127) // 128 * 128                  # right-padded: causality keeps the padding invisible to real positions
        wpe_p = self.wpe_k                              # positions past the table are clamped to its last row
        if Tp > c.block_size:
            wpe_p = torch.cat([wpe_p, wpe_p[-1:].expand(Tp - c.block_size, -1)]).contiguous()
        x = K.embedding_fwd(F.pad(idx, (0, Tp - P)).reshape(-1).contiguous(), self.wte_k, wpe_p, Tp)
        for layer, (params, shadows) in enumerate(self.blocks):
            x = TX.block_prefill(x, (B, Tp, c.n_head, c.eps), shadows, params, cache, layer)
        last = torch.arange(B, device=idx.device) * Tp + pl_dev.long() - 1
        xf, _, _ = K.layernorm_fwd(x.index_select(0, last), self.lnw, self.lnb, c.eps)
        logits = BL.linear_fwd_decode(xf, self.wte_k)
        cache.lens.copy_(pl_dev)
        return logits

    def extend(self, idx, pl_dev):
        """Resume: idx int64 [B][P] are the tokens behind the cache.lens[b] cached ones (row b: its first pl_dev[b]), run
        as Tq = P rounded up to K.EXTEND_TILE rows per sequence at positions lens[b] + j -> bf16 logits [B][V] at each
        row's last token; cache.lens += pl_dev.  The padding rows' keys land past the new lens, where anything may be."""
        c, cache = self.config, self.cache
        B, P = idx.shape
        Tq = -(-P // K.EXTEND_TILE) * K.EXTEND_TILE
        pos = (cache.lens[:, None] + torch.arange(Tq, device=idx.device, dtype=torch.int32)[None, :]).reshape(-1)
        x = K.embedding_decode(F.pad(idx, (0, Tq - P)).reshape(-1).contiguous(), pos.contiguous(), self.wte_k, self.wpe_k)
        for layer, (params, shadows) in enumerate(self.blocks):
            x = TX.block_extend(x, (B, Tq, c.n_head, c.eps), shadows, params, cache, layer)
        last = torch.arange(B, device=idx.device) * Tq + pl_dev.long() - 1
        xf, _, _ = K.layernorm_fwd(x.index_select(0, last), self.lnw, self.lnb, c.eps)
        logits = BL.linear_fwd_decode(xf, self.wte_k)
        cache.lens.add_(pl_dev)
        return logits

    def ingest(self, idx, pl_dev, resume):
        return self.extend(idx, pl_dev) if resume else self.prefill(idx, pl_dev)

    def rows(self, tok, pos, S=1):
        """Row b*S + j: token tok[b*S + j] at position pos[b*S + j] (clamped to the table) and cache slot cache.lens[b] + j
        -> bf16 logits [B*S][V].  No host read-back, no side stream, cache.lens unchanged: capturable as it stands."""
        c = self.config
        conf = (self.B, S, c.n_head, c.eps)
        x = K.embedding_decode(tok, pos, self.wte_k, self.wpe_k)
        for layer, (params, shadows) in enumerate(self.blocks):
            x = TX.block_step(x, conf, shadows, params, self.cache, layer, S)
        xf, _, _ = K.layernorm_fwd(x, self.lnw, self.lnb, c.eps)
        return BL.linear_fwd_decode(xf, self.wte_k) if S == 1 else K.gemm_skinny(xf, self.wte_k)


class Reference:
    """One call's CPU model (plain PyTorch, any head dim), the numerics reference of :class:`Engine`; ``lens`` int64 [B]"""

    def __init__(self, model, B, Tmax):
        self.model, self.c, self.tr = model, model.config, model.transformer
        w, self.H, self.hd = self.tr.wte.weight, self.c.n_head, self.c.n_embd // self.c.n_head
        self.ks = [torch.zeros(B, self.H, Tmax, self.hd, device=w.device, dtype=w.dtype) for _ in self.tr.h]
        self.vs = [torch.zeros_like(k) for k in self.ks]
        self.ar, self.keys, self.lens = torch.arange(B, device=w.device), torch.arange(Tmax, device=w.device), None

    def prefill(self, idx, pl_dev):
        """-> fp32 logits [B][V] at each prompt's last position"""
        c, tr, H, hd = self.c, self.tr, self.H, self.hd
        B, P = idx.shape
        self.lens = pl_dev.long().clone()
        x = tr.wte(idx) + tr.wpe(torch.arange(P, device=idx.device).clamp(max=c.block_size - 1))
        for blk, kc, vc in zip(tr.h, self.ks, self.vs):
            q, k, v = (t.view(B, P, H, hd).transpose(1, 2) for t in blk.attn.c_attn(blk.ln_1(x)).split(c.n_embd, dim=2))
            kc[:, :, :P], vc[:, :, :P] = k, v
            y = F.scaled_dot_product_attention(q, k, v, is_causal=True)
            x = x + blk.attn.c_proj(y.transpose(1, 2).reshape(B, P, c.n_embd))
            x = x + blk.mlp(blk.ln_2(x))
        return self.model.lm_head(tr.ln_f(x[self.ar, self.lens - 1])).float()

    def step(self, tok):
        """tok [B] at position lens[b] -> the next fp32 logits; lens += 1"""
        c, tr, H, hd, ar, lens = self.c, self.tr, self.H, self.hd, self.ar, self.lens
        B = tok.shape[0]
        x = tr.wte(tok) + tr.wpe(lens.clamp(max=c.block_size - 1))                     # [B][D]
        vis = (self.keys[None, :] <= lens[:, None])[:, None, None, :]                   # keys 0..lens[b], new one included
        for blk, kc, vc in zip(tr.h, self.ks, self.vs):
            q, k, v = (t.view(B, H, hd) for t in blk.attn.c_attn(blk.ln_1(x)).split(c.n_embd, dim=1))
            kc[ar, :, lens], vc[ar, :, lens] = k, v
            y = F.scaled_dot_product_attention(q.unsqueeze(2), kc, vc, attn_mask=vis)
            x = x + blk.attn.c_proj(y.reshape(B, c.n_embd))
            x = x + blk.mlp(blk.ln_2(x))
        lens.add_(1)
        return self.model.lm_head(tr.ln_f(x)).float()


def fused_stepper(model, idx, pl_dev, max_new_tokens, graph=False, cache=None, resume=False):
    """GPU: prefill -> (fp32 logits [B][V] at each prompt's last position, step(tok) -> the next logits, in one fp32
    buffer).  The engine of the torch-sampler loop: the token comes from the host side of the loop."""
    B, P = idx.shape
    eng = Engine(model, B, P, max_new_tokens, 1, cache, resume)
    logits16 = eng.ingest(idx, pl_dev, resume)
    tok_buf = torch.zeros(B, dtype=torch.int64, device=idx.device)
    logits = logits16.float()
    logit_buf = torch.empty_like(logits)

    def unit():     # tok_buf -> logit_buf, at position min(lens[b], block_size - 1)
        logit_buf.copy_(eng.rows(tok_buf, eng.cache.lens))
        eng.cache.lens.add_(1)
    run = Replay(unit, graph)

    def step(tok):
        tok_buf.copy_(tok)
        run()
        return logit_buf
    return logits, step


def _device_loop(eng, r, out, logit_buf):
    """The sampling kernel inside the step.  One unit: sample from the bf16 ``logit_buf`` into ``tok_buf``, column P +
    step of ``out`` and the eos flags; the forward into ``logit_buf``; lens += 1, step += 1.  The last token: sample only."""
    dev, lens = logit_buf.device, eng.cache.lens
    tok_buf = torch.zeros(r.B, dtype=torch.int64, device=dev)
    state = torch.tensor([r.seed, 0], dtype=torch.int64, device=dev)
    one = torch.tensor([0, 1], dtype=torch.int64, device=dev)
    finished = torch.zeros(r.B, dtype=torch.uint8, device=dev) if r.eos is not None else None

    def draw():
        K.sample_logits(logit_buf, tok_buf, state, history=out, col0=r.P, finished=finished, eos_token=r.eos, **r.draw)

    def unit():
        draw()
        logit_buf.copy_(eng.rows(tok_buf, lens))
        lens.add_(1)
        state.add_(one)
    run, kept = Replay(unit, r.graph), []
    for i in range(r.N):
        if r.return_logits:
            kept.append(logit_buf.float())
        if i < r.N - 1:
            run()
        else:
            draw()
    return torch.stack(kept, 1) if r.return_logits else None


def _speculate_device(eng, r, pl_dev, out, logit_buf):
    """Token 0 is drawn from the prefill logits; then one unit per verify step: spec_prepare (last token + S - 1 drafts,
    positions, the uniforms of token indices ntok .. ntok + S - 1) -> the forward on B*S rows -> sample with those
    uniforms -> spec_accept (out, ntok, lens, eos flags, done, stats).  The host reads ``done`` after each unit."""
    B, P, N, S = r.B, r.P, r.N, r.S
    dev, lens = logit_buf.device, eng.cache.lens
    state = torch.tensor([r.seed, 0], dtype=torch.int64, device=dev)
    finished = torch.zeros(r.B, dtype=torch.uint8, device=dev) if r.eos is not None else None
    tok_buf = torch.zeros(B, dtype=torch.int64, device=dev)
    K.sample_logits(logit_buf, tok_buf, state, history=out, col0=P, finished=finished, eos_token=r.eos, **r.draw)
    ntok = torch.ones(B, dtype=torch.int32, device=dev)
    tok_in = torch.zeros(B * S, dtype=torch.int64, device=dev)
    t = torch.zeros_like(tok_in)
    pos = torch.zeros(B * S, dtype=torch.int32, device=dev)
    u = torch.zeros(B * S, dtype=torch.float32, device=dev)
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    stats = torch.zeros(S + 1, dtype=torch.int64, device=dev)

    def unit():
        K.spec_prepare(out, P, N, pl_dev, ntok, lens, r.seed, S, tok_in, pos, u, guess=r.guess, ngram=r.ngram)
        K.sample_logits(eng.rows(tok_in, pos, S), t, state, u=u, **r.draw)
        K.spec_accept(tok_in, t, out, P, N, ntok, lens, done, stats, S, finished=finished, eos_token=r.eos)
    run, steps = Replay(unit, r.graph), 0
    while steps < N - 1:
        run()
        steps += 1
        if int(done.item()):
            break
    return {"verify_steps": steps, "stats": stats.tolist()}


def _speculate_reference(model, r, idx, pl_dev, out):
    """CPU: the same loop on ops.speculate's references.  A step's S verify logits come from S successive reference steps
    (a position the row never reaches is clamped to the last slot, which no emitted token reads); then lens = accepted"""
    B, P, N, S = r.B, r.P, r.N, r.S
    Tmax = max(r.pl) + N
    ref = Reference(model, B, Tmax)
    finished = torch.zeros(B, dtype=torch.uint8, device=idx.device) if r.eos is not None else None
    out[:, P], _, _ = sample_reference(ref.prefill(idx, pl_dev), state=(r.seed, 0), finished=finished, eos_token=r.eos,
                                       **r.draw)
    ntok = torch.ones(B, dtype=torch.int32, device=idx.device)
    lens = pl_dev.clone()
    stats = torch.zeros(S + 1, dtype=torch.int64)
    steps = 0
    while steps < N - 1:
        tok_in, _, u = prepare_reference(out, P, N, pl_dev, ntok, lens, r.seed, S, guess=r.guess, ngram=r.ngram)
        t = torch.zeros_like(tok_in)
        for j in range(S):
            ref.lens.copy_((lens.long() + j).clamp(max=Tmax - 1))
            t[j::S], _, _ = sample_reference(ref.step(tok_in[j::S]), u=u[j::S], **r.draw)
        done = accept_reference(tok_in, t, out, P, N, ntok, lens, finished, r.eos, stats, S)
        ref.lens.copy_(lens)
        steps += 1
        if done:
            break
    return {"verify_steps": steps, "stats": stats.tolist()}


def generate(model, idx, max_new_tokens, **kw):
    """``GPT2.generate`` (under its no_grad): the check, then the loop of (speculate, sampler, device)"""
    r = check_args(model.config, idx, max_new_tokens, **kw)
    B, P, N = r.B, r.P, r.N
    idx = idx.long()
    out = torch.cat([idx, idx.new_zeros(B, N)], 1)
    if N == 0 and r.resume:                             # chunked prefill: the ingest is the whole call
        Engine(model, B, P, 0, r.S or 1, r.cache, True).extend(idx, torch.tensor(r.pl, device=idx.device,
                                                                                 dtype=torch.int32))
    if N == 0:
        if r.return_stats:
            return out, {"verify_steps": 0, "stats": [0] * (r.S + 1)}
        return (out, torch.empty(B, 0, model.config.vocab_size, device=idx.device)) if r.return_logits else out
    pl_dev = torch.tensor(r.pl, device=idx.device, dtype=torch.int32)
    if r.guess is not None:
        r = r._replace(guess=r.guess.to(idx.device).contiguous())
    if r.seed is not None and idx.is_cuda:         # the sampling kernel is inside the step: the loop is on the device
        eng = Engine(model, B, P, N, r.S or 1, r.cache, r.resume)
        logit_buf = eng.ingest(idx, pl_dev, r.resume)
        res = _speculate_device(eng, r, pl_dev, out, logit_buf) if r.S else _device_loop(eng, r, out, logit_buf)
        return (out, res) if r.return_logits or r.return_stats else out
    if r.S:
        stats = _speculate_reference(model, r, idx, pl_dev, out)
        return (out, stats) if r.return_stats else out
    # the token is drawn on the host side of the loop: the torch sampler on both devices, the device sampler's reference
    if idx.is_cuda:
        logits, step = fused_stepper(model, idx, pl_dev, N, r.graph, r.cache, r.resume)
    else:
        ref = Reference(model, B, max(r.pl) + N)
        logits, step = ref.prefill(idx, pl_dev), ref.step
    finished = torch.zeros(B, dtype=torch.bool, device=idx.device)      # rows that have emitted eos_token
    if r.seed is not None:                                              # sample_reference: uint8 flags, None without eos
        finished = finished.to(torch.uint8) if r.eos is not None else None
    kept = []
    for i in range(N):
        if r.return_logits:
            kept.append(logits.clone())
        if r.seed is not None:
            tok, _, _ = sample_reference(logits, state=(r.seed, i), finished=finished, eos_token=r.eos, **r.draw)
        else:
            tok = sample(logits, r.draw["temperature"], r.draw["top_k"], r.generator, r.draw["top_p"])
            if r.eos is not None:
                tok = torch.where(finished, torch.full_like(tok, int(r.eos)), tok)
                finished = finished | (tok == int(r.eos))
        out[:, P + i] = tok
        if i + 1 < N:
            logits = step(tok)
    return (out, torch.stack(kept, 1)) if r.return_logits else out


class Session:
    """A conversation of B rows over several ``generate`` calls that keeps the key/value cache between them
    (``GPT2.session``).  Host-side accounting only: ``history[b]`` is every token of row b so far (the turns and the
    emitted tokens, cut after the first ``eos_token`` of each call) and ``cached[b]`` how many of them are in the cache.

    Invariant: slot i of row b of the cache holds the K/V of history[b][i] for every i < cached[b].

    :meth:`generate` packs, for each row, the uncached tail of the history (the last token a call emits is never run
    through the model, so it is cached by the next call) followed by the new turn, and runs ``generate(resume=True)`` on
    it: a turn costs its own tokens against the cache, not the whole history again.  On the CPU there is no cache: the
    same call re-runs ``generate`` on the concatenated history, which is the definition the GPU path is held to."""

    def __init__(self, model, B, max_len, S=1):
        if B < 1 or not 1 <= max_len <= model.config.block_size:
            raise ValueError(f"session: B >= 1 and 1 <= max_len <= block size {model.config.block_size}, got B = {B}, "
                             f"max_len = {max_len}")
        self.model, self.B, self.max_len = model, B, max_len
        self.device = model.transformer.wte.weight.device
        self.history, self.cached = [[] for _ in range(B)], [0] * B
        self.cache = TX.KVCache(model, B, max_len, self.device, S=S) if self.device.type == "cuda" else None

    def generate(self, turns, max_new_tokens, *, eos_token=None, **sampling):
        """``turns``: B token sequences (lists or 1-D tensors), row b's next turn; it may be empty only where the row has
        an uncached tail.  ``sampling``: generate's temperature, top_k, top_p, sampler, seed, speculate, draft, ngram,
        generator, graph.  -> the new tokens per row, B lists, each cut after its first ``eos_token``."""
        if len(turns) != self.B:
            raise ValueError(f"session: {self.B} turns expected, got {len(turns)}")
        for bad in ("cache", "resume", "prompt_lens", "return_logits", "return_stats"):
            if bad in sampling:
                raise ValueError(f"session: {bad} is the session's own argument of generate")
        N = int(max_new_tokens)
        hist = [h + [int(t) for t in (turn.tolist() if torch.is_tensor(turn) else turn)]
                for h, turn in zip(self.history, turns)]
        gpu = self.cache is not None
        rows = [h[n:] for h, n in zip(hist, self.cached)] if gpu else hist
        pl = [len(r) for r in rows]
        if min(pl) < 1 or max(len(h) for h in hist) + N > self.max_len:
            raise ValueError(f"session: every row needs a token to run and history + max_new_tokens <= max_len = "
                             f"{self.max_len}; got {pl} tokens to run, histories of {[len(h) for h in hist]}")
        P = max(pl)
        idx = torch.tensor([r + [0] * (P - len(r)) for r in rows], dtype=torch.int64, device=self.device)
        if gpu:
            out = self.model.generate(idx, N, eos_token=eos_token, prompt_lens=pl, cache=self.cache, resume=True,
                                      **sampling)
        elif N:
            out = self.model.generate(idx, N, eos_token=eos_token, prompt_lens=pl, **sampling)
        else:
            out = idx
        new = [row[P:P + N] for row in out.tolist()]
        if eos_token is not None:
            new = [n[:n.index(int(eos_token)) + 1] if int(eos_token) in n else n for n in new]
        if gpu:     # slots behind the ingested tokens hold the emitted tokens that were run, in order: keep the cut ones
            base = [len(h) for h in hist]
            self.cached = [b0 + max(0, min(len(n), have - b0)) for b0, n, have in zip(base, new, self.cache.lens.tolist())]
            self.cache.truncate(self.cached)
        self.history = [h + n for h, n in zip(hist, new)]
        return new

    def truncate(self, lens):
        """Rewind every row to its first lens[b] tokens (an int: all rows): history and cache.  The last kept token is
        left to the next call to run, as after a call that emitted it: a turn repeated behind the rewound history is
        then the computation it was the first time, and its tokens repeat bitwise."""
        lens = [int(lens)] * self.B if not hasattr(lens, "__len__") else [int(v) for v in lens]
        self.history = [h[:max(n, 0)] for h, n in zip(self.history, lens)]
        self.cached = [min(c, max(len(h) - 1, 0)) for c, h in zip(self.cached, self.history)]
        if self.cache is not None:
            self.cache.truncate(self.cached)
