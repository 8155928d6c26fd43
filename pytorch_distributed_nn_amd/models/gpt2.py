"""GPT-2 (BASELINE.json config 4: "GPT-2-small transformer DDP bf16").  New capability — the reference
trains only CNNs/MLPs — built on the same engine: flat fp32 parameter arena with bf16
shadows (``optim.flat``), RCCL DDP buckets (``parallel.ddp``), fused optimizers.

Architecture = GPT-2 small: 12 layers, 12 heads, d_model 768, context 1024, pre-LN blocks, GELU(tanh)
MLP 4x, learned position embeddings, LM head tied to the token embedding.  The vocabulary is padded from
50257 to 50304 (a multiple of 128: MFMA tile-aligned; the extra rows are never targets).  Parameter names
follow the HuggingFace layout (``transformer.h.0.attn.c_attn.weight`` ...), but Linear weights are stored
[out][in] (nn.Linear), i.e. transposed relative to HF's Conv1D.

GPU path: ``ops.transformer`` fused Functions (one autograd node per block); CPU path: plain PyTorch in
fp32 (tests, and the numerics reference of the GPU path).  ``forward(idx, targets)`` returns the mean
next-token cross-entropy when targets are given (the fused head never materialises fp32 logits),
otherwise the logits.

Packed documents (``GPT2Config.doc_mask_eot`` or ``forward(..., doc_bounds=)``): rows that concatenate several
documents, each ended by an end-of-text token, attend causally inside their own document only (the DOC kernels of
``csrc/kernels/attention.hip``; on the CPU an equivalent boolean mask for SDPA).  The learned absolute positions are
unchanged: position t of the row, not reset at a document start.

Dropout (``embd_pdrop``, ``attn_pdrop``, ``resid_pdrop``; all 0 by default, GPT-2's own value is 0.1): active in a
training forward only (``model.training`` and grad mode on).  No mask is stored: every kernel derives its keep bits from
a (seed, step) pair on the device (``csrc/kernels/dropout_rng.h``), which each training forward snapshots for its own
backward and then advances, so a captured step draws new masks on every replay.  The pair is a plain attribute created
on the input's device at the first training forward, seeded from ``torch.initial_seed()`` and the rank; it is no buffer
and not in ``state_dict``.  The CPU path applies the same bits (``ops.transformer.dropout_keep_reference``).

Generation (``generate``, a delegate to ``generation.py``): one prefill over the prompt, then one single-token step per
new token against a key/value cache (GPU: ``ops.transformer.KVCache`` / ``block_prefill`` / ``block_step``, head dim 64
only; CPU: a plain fp32 cache, the reference of the GPU path).  The document mask is not applied there.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import generation as G
from .. import tuning
from ..ops import functional as OF
from ..ops import transformer as TX
from ..optim.flat import direct_grad


@dataclass
class GPT2Config:
    vocab_size: int = 50304
    block_size: int = 1024
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    eps: float = 1e-5
    fp8: bool = False          # block linears' forward GEMMs in fp8 (e4m3, delayed scaling); bwd bf16
    # training loss only (grad mode on); an evaluation forward returns the plain cross-entropy
    label_smoothing: float = 0.0   # eps: target = (1 - eps) onehot + eps / vocab_size
    z_loss: float = 0.0            # z: + z * logsumexp^2 per token (PaLM)
    # packed documents: the id of the end-of-text token that ends (and belongs to) each document of a row; attention
    # then stays inside the document.  None = plain causal attention over the whole row.  Positions are not reset.
    doc_mask_eot: int | None = None
    # dropout, training forwards only: on wte + wpe, on the attention probabilities (inside the flash kernels: head dim
    # 64 and T % 128 == 0 only), on each branch's output before its residual add.  Quantised to n / 256.
    embd_pdrop: float = 0.0
    attn_pdrop: float = 0.0
    resid_pdrop: float = 0.0


CONFIGS = {
    "gpt2_small": GPT2Config(),
    "gpt2": GPT2Config(),
    "gpt2_medium": GPT2Config(n_layer=24, n_head=16, n_embd=1024),
    "gpt2_large": GPT2Config(n_layer=36, n_head=20, n_embd=1280),
    "gpt2_tiny": GPT2Config(vocab_size=512, block_size=128, n_layer=2, n_head=2, n_embd=128),
}


class Attention(nn.Module):
    def __init__(self, c: GPT2Config):
        super().__init__()
        self.n_head = c.n_head
        self.c_attn = nn.Linear(c.n_embd, 3 * c.n_embd)
        self.c_proj = nn.Linear(c.n_embd, c.n_embd)

    def forward(self, x, mask=None, keep=None):
        B, T, D = x.shape
        q, k, v = self.c_attn(x).split(D, dim=2)
        q, k, v = (t.view(B, T, self.n_head, D // self.n_head).transpose(1, 2) for t in (q, k, v))
        if keep is not None:        # [B][H][T][T]: keep / (1 - p) on the probabilities, after the softmax
            i = torch.arange(T, device=x.device)
            vis = mask if mask is not None else (i[None, :] <= i[:, None])
            att = (q @ k.transpose(-1, -2)) / math.sqrt(D // self.n_head)
            y = (torch.softmax(att.masked_fill(~vis, float("-inf")), -1) * keep) @ v
        elif mask is not None:      # bool [B][1][T][T], True = visible (causal and inside the document)
            y = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
        else:
            y = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        return self.c_proj(y.transpose(1, 2).reshape(B, T, D))


class MLP(nn.Module):
    def __init__(self, c: GPT2Config):
        super().__init__()
        self.c_fc = nn.Linear(c.n_embd, 4 * c.n_embd)
        self.c_proj = nn.Linear(4 * c.n_embd, c.n_embd)

    def forward(self, x):
        return self.c_proj(F.gelu(self.c_fc(x), approximate="tanh"))


class Block(nn.Module):
    def __init__(self, c: GPT2Config):
        super().__init__()
        self.ln_1 = nn.LayerNorm(c.n_embd, eps=c.eps)
        self.attn = Attention(c)
        self.ln_2 = nn.LayerNorm(c.n_embd, eps=c.eps)
        self.mlp = MLP(c)

    def forward(self, x, mask=None, drop=None):
        if drop is None:
            x = x + self.attn(self.ln_1(x), mask)
            return x + self.mlp(self.ln_2(x))
        keep, r1, r2 = drop         # scaled keep factors (or None): probabilities, attention branch, MLP branch
        a = self.attn(self.ln_1(x), mask, keep)
        x = x + (a * r1 if r1 is not None else a)
        m = self.mlp(self.ln_2(x))
        return x + (m * r2 if r2 is not None else m)

    def fp8_metas(self, device):
        metas = getattr(self, "_fp8_metas", None)
        if metas is None:
            from ..ops.fp8 import Fp8Meta
            metas = self._fp8_metas = tuple(Fp8Meta(device) for _ in range(4))
        return metas

    def fused_params(self):
        p = (self.ln_1.weight, self.ln_1.bias, self.attn.c_attn.weight, self.attn.c_attn.bias,
             self.attn.c_proj.weight, self.attn.c_proj.bias, self.ln_2.weight, self.ln_2.bias,
             self.mlp.c_fc.weight, self.mlp.c_fc.bias, self.mlp.c_proj.weight, self.mlp.c_proj.bias)
        shadows = tuple(OF.weight_bf16(w) for w in (p[2], p[4], p[8], p[10]))
        return p, shadows


class GPT2(nn.Module):
    def __init__(self, config: GPT2Config | None = None):
        super().__init__()
        c = self.config = config or GPT2Config()
        self.transformer = nn.ModuleDict(dict(
            wte=nn.Embedding(c.vocab_size, c.n_embd),
            wpe=nn.Embedding(c.block_size, c.n_embd),
            h=nn.ModuleList([Block(c) for _ in range(c.n_layer)]),
            ln_f=nn.LayerNorm(c.n_embd, eps=c.eps),
        ))
        self.lm_head = nn.Linear(c.n_embd, c.vocab_size, bias=False)
        self.lm_head.weight = self.transformer.wte.weight          # tied
        self.apply(self._init)
        for n, p in self.named_parameters():
            if n.endswith("c_proj.weight"):                          # GPT-2 residual-projection scaling
                nn.init.normal_(p, 0.0, 0.02 / math.sqrt(2 * c.n_layer))

    @staticmethod
    def _init(m):
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, 0.0, 0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, 0.0, 0.02)

    def awaits_params(self, idx, *args, **kwargs):
        """The fused GPU forward fetches every block's weight shadows through await_param (OF.weight_bf16), so a
        k-of-n DistributedDataParallel forward is checked before every block without the per-op ParamUseMode
        dispatch (a PS worker still uses ParamUseMode: its LayerNorm / bias parameters must have
        ARRIVED before use, which only the per-op hook guarantees)."""
        return bool(getattr(idx, "is_cuda", False))

    def ddp_tied_rows(self):
        """The tied token-embedding / LM-head weight: DistributedDataParallel all-reduces its dense (LM-head) gradient
        as soon as the head's backward has produced it and gathers the embedding's rows at the end (split_tied)."""
        return self.transformer.wte.weight if self.lm_head.weight is self.transformer.wte.weight else None

    def _row_tail(self):
        ref = self.__dict__.get("_pdnn_row_tail")
        ddp = ref() if ref is not None else None
        return ddp if ddp is not None and ddp._tail is self.transformer.wte.weight else None

    def num_params(self, non_embedding=True):
        n = sum(p.numel() for p in self.parameters())
        return n - self.transformer.wpe.weight.numel() if non_embedding else n

    def flops_per_token(self, T=None):
        """Training FLOPs per token (6N + attention 12*L*D*T, PaLM appendix B accounting)."""
        c = self.config
        T = T or c.block_size
        return 6 * self.num_params() + 12 * c.n_layer * c.n_embd * T

    def _t_weights(self):
        ws = self.__dict__.get("_pdnn_t_ws")
        if ws is None:
            ws = [self.transformer.wte.weight]
            for blk in self.transformer.h:
                ws += [blk.attn.c_attn.weight, blk.attn.c_proj.weight, blk.mlp.c_fc.weight, blk.mlp.c_proj.weight]
            self.__dict__["_pdnn_t_ws"] = ws
        return ws

    def _doc_bounds(self, idx, doc_bounds):
        """(doc_start, doc_end) int32 [B][T] on idx's device, or None: explicit bounds win over config.doc_mask_eot"""
        if doc_bounds is not None:
            ds, de = doc_bounds
            if ds.shape != idx.shape or de.shape != idx.shape:
                raise ValueError(f"doc_bounds: expected two [B][T] = {tuple(idx.shape)} tensors, got {tuple(ds.shape)}, "
                                 f"{tuple(de.shape)}")
            return tuple(t.to(device=idx.device, dtype=torch.int32).contiguous() for t in (ds, de))
        eot = self.config.doc_mask_eot
        if eot is None:
            return None
        if idx.is_cuda:             # one small kernel per forward, no host read-back: the step stays capturable
            from ..ops import kernels as K
            return K.doc_bounds(idx.long().contiguous(), int(eot))
        return TX.doc_bounds_reference(idx, int(eot))

    def dropout_rates(self):
        """(embd, attn, resid) of this forward: the config's in a training forward, else None"""
        c = self.config
        rates = (c.embd_pdrop, c.attn_pdrop, c.resid_pdrop)
        for name, p in zip(("embd_pdrop", "attn_pdrop", "resid_pdrop"), rates):
            if not 0.0 <= p < 1.0:
                raise ValueError(f"GPT2Config.{name} must be in [0, 1), got {p!r}")
        return rates if self.training and torch.is_grad_enabled() and any(rates) else None

    def dropout_state(self, device):
        """The int64 (seed, step) pair the dropout kernels read, on ``device`` (created, or moved, on demand)."""
        st = self.__dict__.get("_pdnn_drop_state")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if st is None or st.device != device:
            pair = st.tolist() if st is not None else [TX.dropout_seed(), 0]
            st = self.__dict__["_pdnn_drop_state"] = torch.tensor(pair, dtype=torch.int64, device=device)
        return st

    def set_dropout_state(self, seed, step=0, device=None):
        """Restart the mask sequence: the next training forward draws the masks of (seed, step)."""
        device = device if device is not None else next(self.parameters()).device
        self.__dict__["_pdnn_drop_state"] = torch.tensor([int(seed) & ((1 << 63) - 1), int(step)], dtype=torch.int64,
                                                         device=device)

    def forward(self, idx, targets=None, doc_bounds=None):
        """``doc_bounds``: optional (doc_start, doc_end), integer [B][T], for callers that pack themselves (first token
        of t's document, one past its last); otherwise config.doc_mask_eot, when set, derives them from ``idx`` once
        per forward on the device, for every block."""
        B, T = idx.shape
        c = self.config
        assert T <= c.block_size, f"sequence length {T} > block size {c.block_size}"
        doc = self._doc_bounds(idx, doc_bounds)
        rates = self.dropout_rates()
        # one snapshot of (seed, step) per training forward, for every Function of it; the live state moves on
        snap = TX.dropout_advance(self.dropout_state(idx.device)) if rates is not None else None
        if not idx.is_cuda:
            return self._forward_reference(idx, targets, doc, (rates, snap) if rates is not None else None)
        tr = self.transformer
        wte, wpe = tr.wte.weight, tr.wpe.weight
        pf = tuning.get("wt_prefetch")
        if pf and targets is not None and torch.is_grad_enabled():
            # the data-gradient GEMMs' transposed weight copies, refreshed in one launch at forward start
            # (instead of ~50 small transposes inside the backward)
            from ..ops.side_stream import side_stream
            OF.prefetch_weight_t(self._t_weights(), side_stream(idx.device) if pf == 2 else None)
        wte_k, wpe_k = OF.weight_bf16(wte), OF.weight_bf16(wpe)
        # tied wte: with targets the fused LM head and the embedding both accumulate into its arena gradient
        hd = targets is not None and direct_grad(wte) is not None
        ddp = self._row_tail() if hd and torch.is_grad_enabled() else None
        edrop = (rates[0], snap) if rates is not None and rates[0] else None
        if ddp is not None:
            # split under DistributedDataParallel: the head announces wte, the embedding's rows go through
            # ddp.reduce_sparse_rows (wte is not an autograd input of the embedding)
            x = TX.EmbeddingFn.apply(idx.reshape(-1).long().contiguous(), T, wte_k, wpe_k, None, wpe, False, (ddp, wte),
                                     edrop)
        else:
            x = TX.EmbeddingFn.apply(idx.reshape(-1).long().contiguous(), T, wte_k, wpe_k, wte, wpe, hd, None, edrop)
        for layer, blk in enumerate(tr.h):
            params, shadows = blk.fused_params()
            metas = blk.fp8_metas(x.device) if c.fp8 else None
            drop = (rates[1], rates[2], snap, layer) if rates is not None and (rates[1] or rates[2]) else None
            x = TX.GPT2BlockFn.apply(x, TX.BlockConf(B, T, c.n_head, c.eps, metas, doc, drop), shadows, *params)
        if targets is None:
            xf = TX.layer_norm(x, tr.ln_f.weight, tr.ln_f.bias, c.eps)
            return OF.linear(xf, wte).view(B, T, -1)
        train = torch.is_grad_enabled()
        return TX.LMHeadLossFn.apply(x, targets.reshape(-1).long().contiguous(), c.eps, wte_k, tr.ln_f.weight,
                                     tr.ln_f.bias, wte, hd, ddp is not None, train,
                                     c.label_smoothing if train else 0.0, c.z_loss if train else 0.0)

    # ------------------------------------------------------------------------------------------ generation
    @staticmethod
    def kv_cache_len(P, max_new_tokens):
        """Tmax of the GPU cache for prompts of P columns: the prefill writes the prompt padded to a multiple of 128"""
        return max((P + 127) // 128 * 128, P + max_new_tokens)

    _sample = staticmethod(G.sample)

    @torch.no_grad()
    def generate(self, idx, max_new_tokens, *, temperature=1.0, top_k=None, eos_token=None, prompt_lens=None,
                 generator=None, graph=False, return_logits=False, cache=None, top_p=None, sampler="torch", seed=None,
                 speculate=None, draft="ngram", ngram=3, return_stats=False, resume=False):
        """Sample ``max_new_tokens`` tokens after the prompts ``idx`` int [B][P] with a key/value cache: one prefill over
        the prompt, then one single-token step per new token (GPU: ``ops.transformer.block_step`` on the decode
        attention kernel of ``csrc/kernels/attention_decode.hip``; CPU: plain PyTorch in fp32 with per-layer k, v lists,
        any head dim, the numerics reference of the GPU path).  Runs under no_grad with evaluation semantics (no dropout)
        and leaves the model as it found it.

        ``prompt_lens`` int [B] (default: the full row) lets a batch mix prompt lengths: row b's prompt is
        idx[b, :prompt_lens[b]], the rest of the row is padding.  Returns tokens int64 [B][P + max_new_tokens]: ``idx``
        followed by the new tokens of every row in columns P.. (for a short prompt they continue idx[b, :prompt_lens[b]],
        not the padding); with ``return_logits`` also the fp32 logits [B][max_new_tokens][V] each token was drawn from.

        Sampling: ``temperature == 0`` or ``top_k == 1`` is argmax; otherwise temperature, then top-k, then
        torch.multinomial with ``generator`` (eager torch on the step's logits, outside any captured region).  A row that
        has emitted ``eos_token`` keeps emitting it (device-side mask; the loop always runs max_new_tokens steps and never
        reads the device from the host).  ``graph=True`` (GPU): after one eager warm-up step one decode step is captured
        with torch.cuda.graph on a single stream and replayed; the cache length lives on the device, so a replay follows
        it.  ``cache`` (GPU): an ``ops.transformer.KVCache`` of this batch size with Tmax >= kv_cache_len(P,
        max_new_tokens) to reuse; it is reset first.  ``config.doc_mask_eot`` is not applied: a prompt is one document.
        The block linears are bf16 even with ``config.fp8``.

        ``top_p`` (both samplers): nucleus sampling after top-k.  ``sampler="device"`` draws with the counter-based
        generator instead of ``generator``: step i of row b uses u(``seed``, i, b), and the token is the one defined in
        the header of ``csrc/kernels/sample.hip`` (GPU: that kernel, on the step's bf16 logits, writing the token, the
        output column and the eos flags on the device; CPU: ``ops.sampling.sample_reference`` on the fp32 logits).  The
        tokens are reproducible from ``seed``.  With ``graph=True`` the kernel is part of the captured step (sample ->
        embedding -> blocks -> ln_f -> LM head -> lens += 1, step += 1): the loop issues one replay per token.

        ``speculate=S`` (2 <= S <= 8; needs ``sampler="device"``): speculative decoding.  One verify step runs the last
        emitted token and S - 1 draft tokens of every row through the model at once (GPU: ``ops.transformer.
        block_step`` on the multi-query decode attention kernel, every linear on the skinny GEMM, whose row bits do not
        depend on the row count), draws the target's own token at each of the S positions with u(seed, token index, b),
        and emits the drawn tokens up to and including the first one that differs from its draft.  The returned tokens
        are therefore bit for bit those of ``speculate=None`` with the same seed, whatever the drafts were.  ``draft``:
        ``"ngram"`` (prompt lookup: the continuation of the latest earlier occurrence of the last ``ngram`` .. 1 tokens
        of the row's history) or an int64 [B][max_new_tokens] tensor of guesses for the new tokens.  On the GPU a verify
        step is one unit (csrc/kernels/speculate.hip prepare -> embedding -> blocks -> ln_f -> LM head -> sample ->
        accept) that allocates nothing after the warm-up and is captured and replayed with ``graph=True``; the host
        reads one int32 (all rows complete) after each unit, the only read-back, and stops: at most max_new_tokens - 1
        units.  The GPU path needs tuning ``decode_skinny``, B <= 8 and B * S <= 64; a passed ``cache`` needs ``S`` >= S
        and Tmax >= kv_cache_len(P, max_new_tokens + S) (rejected drafts occupy slots past the accepted length).
        ``return_logits`` is not available with ``speculate``.  ``return_stats=True`` appends a dict: ``verify_steps``
        and ``stats``, where stats[e] counts the (row, verify step) pairs of incomplete rows that emitted e tokens.

        ``resume=True`` (GPU, needs ``cache``): the cache is kept, not reset.  idx[b, :prompt_lens[b]] are the tokens that
        follow the cache.lens[b] cached ones; they are ingested by ``Engine.extend`` (``ops.transformer.block_extend`` on
        the append + extend kernels of ``csrc/kernels/attention_extend.hip``: many queries at an offset against the
        cache) instead of the prefill, and every sampler loop above runs unchanged on top.  ``max_new_tokens == 0`` still
        ingests, so a long prompt can be fed in chunks.  cache.lens is read to the host once, before the first launch:
        every row needs lens[b] + prompt_lens[b] + max_new_tokens (+ S) <= min(block size, cache.Tmax).  Afterwards
        cache.lens counts the tokens that were run (the last emitted token is not among them); :meth:`session` keeps
        that account over several turns."""
        return G.generate(self, idx, max_new_tokens, temperature=temperature, top_k=top_k, eos_token=eos_token,
                          prompt_lens=prompt_lens, generator=generator, graph=graph, return_logits=return_logits,
                          cache=cache, top_p=top_p, sampler=sampler, seed=seed, speculate=speculate, draft=draft,
                          ngram=ngram, return_stats=return_stats, resume=resume)

    def session(self, B, max_len, S=1):
        """A :class:`generation.Session`: B conversations of up to ``max_len`` tokens whose key/value cache is kept from
        one ``session.generate(turns, max_new_tokens, ...)`` to the next (``S``: the largest ``speculate`` to be used)"""
        return G.Session(self, B, max_len, S)

    def _forward_reference(self, idx, targets=None, doc=None, drop=None):
        B, T = idx.shape
        mask = TX.doc_visible(doc[0]).unsqueeze(1) if doc is not None else None
        c = self.config

        def keep(p, site, **shape):     # the kernels' bits for this site, times 1 / (1 - p_eff); None for p = 0
            if not p:
                return None
            bits = TX.dropout_keep_reference(drop[1], site, p, device=idx.device, **shape)
            return bits.to(tr.wte.weight.dtype) * TX.dropout_scale(p)
        tr = self.transformer
        pos = torch.arange(T, device=idx.device)
        ddp = self._row_tail() if targets is not None and torch.is_grad_enabled() else None
        if ddp is not None:     # split tied embedding (see forward): the rows reach wte through the DDP tail
            x = _RowTailEmbedding.apply(idx, tr.wte.weight.detach(), tr.wpe(pos), (ddp, tr.wte.weight))
        else:
            x = tr.wte(idx) + tr.wpe(pos)
        if drop is None:
            for blk in tr.h:
                x = blk(x, mask)
        else:
            pe, pa, pr = drop[0]
            ke = keep(pe, TX.SITE_EMBD, rows=(B * T, c.n_embd))
            if ke is not None:
                x = x * ke.view(B, T, -1)
            for layer, blk in enumerate(tr.h):
                r1, r2 = (keep(pr, 4 * layer + s, rows=(B * T, c.n_embd)) for s in (1, 2))
                x = blk(x, mask, (keep(pa, 4 * layer, attn=(B, c.n_head, T)),
                                  r1.view(B, T, -1) if r1 is not None else None,
                                  r2.view(B, T, -1) if r2 is not None else None))
        logits = self.lm_head(tr.ln_f(x))
        if targets is None:
            return logits
        lg, t = logits.float().view(-1, logits.shape[-1]), targets.reshape(-1)
        if not torch.is_grad_enabled() or not (c.label_smoothing or c.z_loss):
            return F.cross_entropy(lg, t)
        loss = F.cross_entropy(lg, t, label_smoothing=c.label_smoothing)
        if c.z_loss:
            ok = t != -100
            loss = loss + c.z_loss * (torch.logsumexp(lg, -1) ** 2 * ok).sum() / ok.sum().clamp_min(1)
        return loss


class _RowTailEmbedding(torch.autograd.Function):
    """x = table[idx] + pos (reference path): the table is a detached view of the tied wte, so autograd's only edge
    into wte is the LM head's; the embedding rows reach wte.grad through DistributedDataParallel.reduce_sparse_rows
    in the backward.  ``pos`` [T][D] carries the autograd edge (its gradient is g summed over the batch); ``tail`` =
    (ddp, wte) is a tuple so that autograd adds no edge into wte (which would hold wte's AccumulateGrad -- and with it
    DDP's bucket 0 -- until this node has run)."""

    @staticmethod
    def forward(ctx, idx, table, pos, tail):
        ctx.save_for_backward(idx)
        ctx.ddp, ctx.wte = tail
        return F.embedding(idx, table) + pos

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        ddp, wte = ctx.ddp, ctx.wte
        ctx.ddp = ctx.wte = None
        gw = wte.grad
        ddp.reduce_sparse_rows(wte, idx, g, lambda i, r, sc: gw.index_add_(0, i, r.to(gw.dtype), alpha=sc))
        return None, None, g.sum(0), None


def build_gpt2(name: str = "gpt2_small", **kw) -> GPT2:
    base = CONFIGS[name.lower()]
    cfg = GPT2Config(**{**base.__dict__, **kw})
    return GPT2(cfg)
