"""Fused flat-buffer optimizers: SGD (momentum / dampening / weight decay / Nesterov), Adam / AdamW, and the
layer-wise LARS / LAMB (SGD / Adam under a per-tensor trust ratio, ``optim_layerwise.hip``).

torch.optim-compatible API (``param_groups``, ``zero_grad``, ``state_dict``/``load_state_dict``,
``step(closure)``), semantics identical to ``torch.optim.SGD`` / ``Adam`` / ``AdamW``.

When a param group covers a contiguous range of a :class:`~.flat.FlatParams` arena (the normal case:
``SGD(model.parameters())`` after ``flatten_module``/DDP) the whole group is ONE kernel launch
(``optim.hip``) that also refreshes the bf16 weight shadow and applies the gradient averaging factor
(``grad_scale``, or a device-side scale such as 1/alive-count for the straggler-tolerant modes).  Groups
that are not flat fall back to one launch per tensor (GPU) or the torch reference update (CPU).
``set_grad_clip(max_norm)`` adds global-norm gradient clipping to the same step: two norm launches leave the
clip coefficient in device memory and the update launch applies it (the gradient buffer is not rewritten).

Every optimizer here is three pieces under the one ``step()`` of ``_FusedBase``: ``_begin_ranges`` (create the
flat state, advance the step counter), ``_apply_range`` (the kernel launches) and ``_step_param`` (the same rule
in torch ops).  The state and the torch-op recurrences of the two families live once, in ``_MomentumRule`` (SGD,
LARS) and ``_MomentsRule`` (Adam, AdamW, LAMB).

Reference parity: the PS master applies ``param -= lr * avg_grad`` (sync_replicas_master_nn.py:22-28,
216-219) and ignores --momentum (defect D9); the C++ master fuses the average into the update as
``ApplyGrad(lr / count)`` (sync_replicas_master_nn.h:124-128); the TF stack uses Adam
(distributed_train.py:160).  Here momentum IS honoured and the average is fused the C++ way.
"""
from __future__ import annotations

import math

import torch

from .flat import FlatParams


def _flat_of(params):
    fps = {id(getattr(p, "_pdnn_flat", None)) for p in params}
    if len(fps) != 1:
        return None, None
    fp = getattr(params[0], "_pdnn_flat", None)
    if fp is None:
        return None, None
    rng = fp.param_range(params)
    return (fp, rng) if rng is not None else (None, None)


def _cut(t, a, b):
    """``t[a:b]`` of an optional flat tensor; ``t`` itself when that is all of it (same pointer and length for the
    kernel, and the step of a whole arena spends no host time on views)."""
    return t if t is None or (a == 0 and b == t.numel()) else t[a:b]


class _FusedBase(torch.optim.Optimizer):
    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self.grad_scale = 1.0          # host-side factor (e.g. 1/world_size when grads are summed)
        self.grad_scale_dev = None     # optional device scalar (e.g. 1/alive for k-of-n)
        self._flat_cache = {}
        self._graph = False            # graph mode: per-step hyper-parameters live in device memory
        self._hyper = {}
        self._clip = None              # set_grad_clip(): max global L2 norm of the gradient, None = off
        self._clip_out = None          # [norm, coefficient, non-finite flag], written by every clipped step()
        self._clip_ws = None           # the norm kernel's partials (GPU only)

    def _group_flat(self, gi, group):
        if gi not in self._flat_cache:
            self._flat_cache[gi] = _flat_of(group["params"])
        return self._flat_cache[gi]

    # ------------------------------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._consume_overlap():
            return loss
        gsd = self._clip_scale()
        for gi, group in enumerate(self.param_groups):
            fp, rng = self._group_flat(gi, group)
            if fp is not None and fp.data.is_cuda:
                state = self._begin_ranges(gi, group)
                self._apply_range(gi, group, rng[0], rng[1], state, gsd, self._hyper[gi] if self._graph else None)
                fp.generation += 1
                continue
            rows = [self._step_param(group, p, gsd) for p in group["params"] if p.grad is not None]
            if rows and rows[0] is not None:         # LARS / LAMB: (ratio, ||w||, other norm) of every parameter
                self._lw_loose[gi] = torch.stack([torch.stack(r) for r in rows], dim=1)
        return loss

    def _begin_ranges(self, gi, group):
        """Host side, once per step of a flat group: create its state on first use and advance the step counter
        (in graph mode ``pre_replay`` advances it).  Returns what ``_apply_range`` needs of it."""
        raise NotImplementedError

    def _apply_range(self, gi, group, a, b, state, gsd, hyper=None):
        """The kernel launches that update flat-arena elements [a, b) of group ``gi``: the only caller of each
        update kernel.  ``gsd`` is the device gradient scale, ``hyper`` the graph-mode device values."""
        raise NotImplementedError

    def _step_param(self, group, p, gsd):
        """The same update of one parameter in torch ops (loose tensors, CPU arenas)."""
        raise NotImplementedError

    def _scaled_grad(self, p, gsd):
        """The gradient as the update sees it: times ``grad_scale`` and the device scale / clip coefficient."""
        g = p.grad
        if self.grad_scale != 1.0:
            g = g * self.grad_scale
        if gsd is not None:
            g = g * gsd.to(g.device).reshape(())
        return g

    # ------------------------------------------------------------------------------- gradient clipping
    def set_grad_clip(self, max_norm: float | None):
        """Clip the gradient to a global L2 norm of ``max_norm`` inside ``step()``; ``None`` or 0 turns it off
        (the step is then exactly the unclipped one).

        The norm is taken over every param group (and arena) of this optimizer, of the gradient as the update
        sees it (times ``grad_scale`` and ``grad_scale_dev``), with ``torch.nn.utils.clip_grad_norm_``'s formula
        ``coef = min(1, max_norm / (norm + 1e-6))``.  Unlike torch's in-place clip the gradient buffer is NOT
        modified: a norm kernel reads it once and writes the coefficient to device memory, and the fused update
        kernels apply it through the device scale they already read.  No host sync, capturable in a hipGraph.
        Groups that are not flat ranges on a GPU (CPU arenas, loose tensors, more than 8 ranges) compute the same
        formula with torch ops.  ``grad_norm`` / ``grad_nonfinite`` hold the last step's norm and whether it was
        inf/NaN (the step is not skipped then: the coefficient is what the formula gives, as torch with
        ``error_if_nonfinite=False``)."""
        self._clip = float(max_norm) if max_norm else None
        if self._clip is not None:
            self._clip_alloc()

    def _clip_alloc(self):
        # outside any graph capture (set_grad_clip / graph_mode), for the reason _hyper is: a buffer created inside
        # a capture belongs to the graph's pool
        if self._clip_out is not None:
            return
        from ..ops.kernels import CLIP_WS
        dev = self.param_groups[0]["params"][0].device
        self._clip_out = torch.zeros(3, dtype=torch.float32, device=dev)
        if dev.type == "cuda":
            self._clip_ws = torch.zeros(CLIP_WS, dtype=torch.float32, device=dev)

    @property
    def grad_norm(self):
        """Device scalar: the clipped step's global gradient norm (None before clipping was ever set)."""
        return None if self._clip_out is None else self._clip_out[0]

    @property
    def grad_nonfinite(self):
        """Device scalar: 1.0 when the last clipped step's norm was inf or NaN, else 0.0."""
        return None if self._clip_out is None else self._clip_out[2]

    @torch.no_grad()
    def _clip_scale(self):
        """The device gradient scale of this step's update kernels: ``grad_scale_dev`` without clipping, else the
        clip coefficient (with ``grad_scale_dev`` folded in), computed here from the current gradients."""
        if self._clip is None:
            return self.grad_scale_dev
        from ..ops.kernels import CLIP_RANGES
        out = self._clip_out
        flats = [self._group_flat(gi, g) for gi, g in enumerate(self.param_groups)]
        if (self._clip_ws is not None and len(flats) <= CLIP_RANGES
                and all(fp is not None and fp.grad.device == out.device for fp, _ in flats)):
            from ..ops import kernels as K
            nparts = 0
            for fp, (s, e) in flats:
                nparts += K.sumsq_partials(fp.grad[s:e], self._clip_ws, nparts)
            K.clip_coef(self._clip_ws, nparts, self._clip, out, self.grad_scale, self.grad_scale_dev)
            return out[1:2]
        norms = []
        for (fp, rng), group in zip(flats, self.param_groups):
            # what the group's update will read: the arena range (fused launch) or the parameters' own .grad
            gs = ([fp.grad[rng[0]:rng[1]]] if fp is not None and fp.data.is_cuda
                  else [p.grad for p in group["params"] if p.grad is not None])
            norms += [torch.linalg.vector_norm(g).to(out.device) for g in gs]
        dev = self.grad_scale_dev.to(out.device).reshape(()) if self.grad_scale_dev is not None else 1.0
        norm = torch.linalg.vector_norm(torch.stack(norms)) if norms else torch.zeros((), device=out.device)
        norm = norm * abs(self.grad_scale * dev)
        out[0] = norm
        out[1] = dev * torch.clamp(self._clip / (norm + 1e-6), max=1.0)
        out[2] = (~torch.isfinite(norm)).float()
        return out[1:2]

    # ---------------------------------------------------------------------------------- graph mode
    # A hipGraph captured around ``step()`` replays the kernels with the arguments they had at capture.
    # In graph mode the fused kernels read the values that change between steps (lr; Adam's bias
    # corrections) from a per-group device buffer instead, and :meth:`pre_replay` — called on the host
    # before every replay — advances the host-side state and refreshes that buffer with stream-ordered
    # fills (no host<->device sync, so the CPU can run ahead of the GPU as in eager mode).
    _HYPER_LEN = 1

    def graph_mode(self, on: bool = True):
        if on:
            for gi, group in enumerate(self.param_groups):
                fp, _ = self._group_flat(gi, group)
                if fp is None or not fp.data.is_cuda:
                    raise RuntimeError("graph mode needs every param group on a flat CUDA arena")
                self._check_graphable(gi)
                # allocated (and filled) OUTSIDE any capture: a buffer created inside the capture would
                # come from the graph pool and its initialising fill would be replayed over pre_replay's
                if gi not in self._hyper:
                    self._hyper[gi] = torch.zeros(self._HYPER_LEN, dtype=torch.float32, device=fp.data.device)
                    self._fill_hyper(gi, group, advance=False)
            if self._clip is not None:
                self._clip_alloc()
        self._graph = bool(on)

    def _check_graphable(self, gi):
        pass

    def _hyper_values(self, gi, group, advance=True):    # one step's values, in the kernel's hyper[] order
        return [group["lr"]]

    @torch.no_grad()
    def _fill_hyper(self, gi, group, advance=True):
        h = self._hyper[gi]
        for j, v in enumerate(self._hyper_values(gi, group, advance)):
            h[j:j + 1].fill_(float(v))

    @torch.no_grad()
    def pre_replay(self):
        for gi, group in enumerate(self.param_groups):
            if gi in self._hyper:
                self._fill_hyper(gi, group)

    # ------------------------------------------------------------------ overlapped step (DDP per bucket)
    # DistributedDataParallel.overlap_optimizer(opt): the update of each gradient bucket is applied on an
    # optimizer stream as soon as the bucket's all-reduce has completed, while the backward of the earlier layers
    # still runs; the step() that follows the backward then has nothing left to do.  One param group on the flat
    # arena, eager (not graph) mode.
    def _overlap_ok(self):
        if self._graph or len(self.param_groups) != 1:
            return None
        if self._clip is not None:     # a per-bucket update cannot know the global norm
            return None
        fp, rng = self._group_flat(0, self.param_groups[0])
        if fp is None or not fp.data.is_cuda:
            return None
        return fp, rng

    @torch.no_grad()
    def _overlap_begin(self):
        """Host side, once per step before the first range: advance the step state (and create it)."""
        self._ovl_state = self._begin_ranges(0, self.param_groups[0])
        self._ovl_done = False

    @torch.no_grad()
    def _overlap_range(self, a, b):
        """Update flat-arena elements [a, b) (a bucket) with the state _overlap_begin prepared (current stream)."""
        self._apply_range(0, self.param_groups[0], a, b, self._ovl_state, self.grad_scale_dev)

    def _overlap_end(self):
        fp, _ = self._group_flat(0, self.param_groups[0])
        fp.generation += 1
        self._ovl_done = True          # the next step() finds the update applied

    def _consume_overlap(self):
        if getattr(self, "_ovl_done", False):
            self._ovl_done = False
            return True
        return False

    def zero_grad(self, set_to_none: bool = False):
        done = set()
        for group in self.param_groups:
            for p in group["params"]:
                fp = getattr(p, "_pdnn_flat", None)
                if fp is not None:
                    if id(fp) not in done:
                        fp.zero_grad()
                        done.add(id(fp))
                elif p.grad is not None:
                    if set_to_none:
                        p.grad = None
                    else:
                        p.grad.detach_()
                        p.grad.zero_()


class _MomentumRule:
    """State and torch-op recurrence of the momentum family (SGD, LARS); mixed in ahead of the optimizer base."""

    def _check_graphable(self, gi):
        # the first momentum step initialises the buffer (a different kernel branch): run it eagerly
        if self.param_groups[gi]["momentum"] != 0 and "momentum_buffer" not in self.state.get(f"flat{gi}", {}):
            raise RuntimeError(f"{type(self).__name__} graph mode: run one eager step before capture "
                               "(momentum buffer init)")

    def _begin_ranges(self, gi, group):         # -> (momentum buffer of the range or None, first step)
        st = self.state[f"flat{gi}"]
        first = "momentum_buffer" not in st
        if group["momentum"] != 0 and first:
            fp, (s, e) = self._group_flat(gi, group)
            st["momentum_buffer"] = torch.zeros(e - s, device=fp.data.device)
        return st.get("momentum_buffer"), first

    def _momentum(self, group, p, d):
        """torch.optim.SGD's momentum / dampening / Nesterov recurrence on the direction ``d`` of parameter ``p``."""
        mom = group["momentum"]
        if mom == 0:
            return d
        st = self.state[p]
        if "momentum_buffer" not in st:
            st["momentum_buffer"] = d.clone().detach()
        else:
            st["momentum_buffer"].mul_(mom).add_(d, alpha=1 - group["dampening"])
        b = st["momentum_buffer"]
        return d.add(b, alpha=mom) if group["nesterov"] else b


class _MomentsRule:
    """State, graph-mode values and torch-op moment update of the Adam family (Adam, AdamW, LAMB); mixed in ahead
    of the optimizer base."""
    _HYPER_LEN = 3

    def _hyper_values(self, gi, group, advance=True):
        st = self.state.setdefault(f"flat{gi}", {})
        if advance:
            st["step"] = st.get("step", 0) + 1       # this replay is step t
        t = max(st.get("step", 0), 1)
        b1, b2 = group["betas"]
        return [group["lr"], 1 - b1 ** t, 1 - b2 ** t]

    def _begin_ranges(self, gi, group):         # -> (m, v of the range, step count t)
        st = self.state[f"flat{gi}"]
        if "step" not in st:
            fp, (s, e) = self._group_flat(gi, group)
            st["step"] = 0
            st["exp_avg"] = torch.zeros(e - s, device=fp.data.device)
            st["exp_avg_sq"] = torch.zeros(e - s, device=fp.data.device)
        if not self._graph:                      # in graph mode t advances in pre_replay(); kernels read hyper[]
            st["step"] += 1
        return st["exp_avg"], st["exp_avg_sq"], max(st["step"], 1)

    def _moments(self, group, p, g):
        """Advance the moments of parameter ``p`` by the gradient ``g``; returns (m, sqrt(v / (1 - b2^t)) + eps,
        1 - b1^t), in torch.optim.Adam's operation order."""
        b1, b2 = group["betas"]
        st = self.state[p]
        if "step" not in st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p)
            st["exp_avg_sq"] = torch.zeros_like(p)
        st["step"] += 1
        t = st["step"]
        st["exp_avg"].lerp_(g, 1 - b1)
        st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (st["exp_avg_sq"].sqrt() / math.sqrt(1 - b2 ** t)).add_(group["eps"])
        return st["exp_avg"], denom, 1 - b1 ** t


class SGD(_MomentumRule, _FusedBase):
    def __init__(self, params, lr=0.01, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov))

    def _apply_range(self, gi, group, a, b, state, gsd, hyper=None):
        from ..ops import kernels as K
        fp, (s, _) = self._group_flat(gi, group)
        buf, first = state
        K.sgd_step(_cut(fp.data, a, b), _cut(fp.grad, a, b), _cut(buf, a - s, b - s), _cut(fp.shadow, a, b),
                   group["lr"], group["momentum"], group["dampening"], group["weight_decay"], group["nesterov"],
                   gsd, self.grad_scale, first, hyper=hyper)

    def _step_param(self, group, p, gsd):
        g = self._scaled_grad(p, gsd)
        if group["weight_decay"] != 0:
            g = g.add(p, alpha=group["weight_decay"])
        p.add_(self._momentum(group, p, g), alpha=-group["lr"])


class Adam(_MomentsRule, _FusedBase):
    decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _apply_range(self, gi, group, a, b, state, gsd, hyper=None):
        from ..ops import kernels as K
        fp, (s, _) = self._group_flat(gi, group)
        m, v, t = state
        b1, b2 = group["betas"]
        K.adam_step(_cut(fp.data, a, b), _cut(fp.grad, a, b), _cut(m, a - s, b - s), _cut(v, a - s, b - s),
                    _cut(fp.shadow, a, b), group["lr"], b1, b2, group["eps"], group["weight_decay"], self.decoupled,
                    1 - b1 ** t, 1 - b2 ** t, gsd, self.grad_scale, hyper=hyper)

    def _step_param(self, group, p, gsd):
        lr, wd = group["lr"], group["weight_decay"]
        g = self._scaled_grad(p, gsd)
        if self.decoupled:
            p.mul_(1 - lr * wd)
        elif wd:
            g = g.add(p, alpha=wd)
        m, denom, bc1 = self._moments(group, p, g)
        p.addcdiv_(m, denom, value=-lr / bc1)


class AdamW(Adam):
    decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
        super().__init__(params, lr, betas, eps, weight_decay)


# ------------------------------------------------------------------------------------ layer-wise: LARS / LAMB
def _exclude_1d(p):
    """The default ``exclude`` of LARS / LAMB: biases and normalisation gains (every parameter of at most 1-D)."""
    return p.ndim <= 1


class _LayerwiseBase(_FusedBase):
    """SGD / Adam under a per-tensor trust ratio.  A param group on a contiguous GPU arena range is three launches
    (optim_layerwise.hip): per-chunk norm partials, per-segment ratios, per-chunk update + bf16 shadow.  The
    kernels know where each parameter begins and ends (segment / chunk tables, derived data cached per group like
    ``_hyper``), so the arena's alignment padding is neither read into a norm nor written.  Loose tensors and CPU
    arenas run the same formulas per parameter in torch ops.

    ``exclude(p)`` -> True leaves a parameter out of weight decay and out of the scaling (ratio 1); ``None`` adapts
    and decays everything.  ``trust_ratios(gi)`` / ``param_norms(gi)`` / ``update_norms(gi)`` return the last
    step's per-parameter values of group ``gi``, in group order, as a device vector (no sync)."""

    def __init__(self, params, defaults, exclude):
        super().__init__(params, defaults)
        self._exclude = exclude
        self._lw = {}                  # gi -> tables, workspace, result of the fused path
        self._lw_loose = {}            # gi -> [3, nparams] result of the torch-op path

    def _excluded(self, p):
        return self._exclude is not None and bool(self._exclude(p))

    def _overlap_ok(self):             # a bucket holds parts of tensors: no per-bucket trust ratio
        return None

    # tables, workspace and result vector of group gi; built on first use and whenever the group's weight decay
    # changes -- outside any graph capture (graph_mode() calls this, as it allocates _hyper)
    def _lw_prepare(self, gi, group):
        from ..ops import kernels as K
        fp, (s, e) = self._group_flat(gi, group)
        wd = float(group["weight_decay"])
        lw = self._lw.get(gi)
        if lw is not None and lw["wd"] == wd:
            return lw
        idx = [p._pdnn_flat_idx for p in group["params"]]
        order = sorted(range(len(idx)), key=lambda j: idx[j])          # table (arena) order -> group position
        segs = []
        for j in order:
            p = group["params"][j]
            ex = self._excluded(p)
            segs.append((fp.offsets[idx[j]] - s, p.numel(), 0.0 if ex else wd, not ex))
        tab = K.LwTables(segs, e - s, fp.data.device)
        ws, out = tab.workspace()
        perm = None
        if order != list(range(len(idx))):
            inv = [0] * len(order)
            for t, j in enumerate(order):
                inv[j] = t
            perm = torch.tensor(inv, dtype=torch.long, device=fp.data.device)
        lw = self._lw[gi] = dict(wd=wd, tab=tab, ws=ws, out=out, perm=perm)
        return lw

    def graph_mode(self, on: bool = True):
        if on:
            for gi, group in enumerate(self.param_groups):
                fp, _ = self._group_flat(gi, group)
                if fp is not None and fp.data.is_cuda:
                    self._lw_prepare(gi, group)
        super().graph_mode(on)

    def _lw_result(self, gi, row):
        lw = self._lw.get(gi)
        if lw is not None:
            n = lw["tab"].nseg
            v = lw["out"][row * n:(row + 1) * n]
            return v if lw["perm"] is None else v.index_select(0, lw["perm"])
        res = self._lw_loose.get(gi)
        return None if res is None else res[row]

    def trust_ratios(self, gi: int = 0):
        """Device vector: the last step's trust ratio of every parameter of group ``gi`` (None before a step)."""
        return self._lw_result(gi, 0)

    def param_norms(self, gi: int = 0):
        """Device vector: ||w|| of every parameter of group ``gi`` in front of the last step."""
        return self._lw_result(gi, 1)

    def update_norms(self, gi: int = 0):
        """Device vector: the norm under the last step's ratios: the gradient's as the update saw it (LARS), or
        that of u = m^ / (sqrt(v^) + eps) + wd w (LAMB)."""
        return self._lw_result(gi, 2)

    def _ratio(self, wn, un, r, adapt, clamp):
        """The kernels' rule in torch ops: 1 unless adapted with both norms non-zero; a NaN norm gives NaN."""
        if not adapt:
            return torch.ones_like(wn)
        if clamp:
            r = torch.where(r > 1, torch.ones_like(r), r)
        return torch.where((wn == 0) | (un == 0), torch.ones_like(wn), r)


class LARS(_MomentumRule, _LayerwiseBase):
    """Layer-wise adaptive rate scaling (You, Gitman, Ginsburg 2017) on SGD's momentum recurrence:

        r = trust_coef * ||w|| / (||g|| + wd * ||w|| + eps)        (g as the update sees it: scaled, clipped)
        d = r * (g + wd * w);   then SGD's momentum / dampening / Nesterov on d;   w -= lr * (...)

    per parameter; r = 1 for an excluded parameter (which also gets no weight decay), when ||w|| = 0 or ||g|| = 0;
    ``clamp`` caps r at 1 (LARC)."""

    def __init__(self, params, lr, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False, trust_coef=1e-3,
                 eps=1e-8, clamp=False, exclude=_exclude_1d):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, trust_coef=trust_coef, eps=eps, clamp=clamp), exclude)

    def _apply_range(self, gi, group, s, e, state, gsd, hyper=None):        # always the group's whole range
        from ..ops import kernels as K
        fp, _ = self._group_flat(gi, group)
        lw = self._lw_prepare(gi, group)
        buf, first = state
        tab, n = lw["tab"], lw["tab"].nseg
        p, g = _cut(fp.data, s, e), _cut(fp.grad, s, e)
        K.lw_norm_partials(p, g, tab, lw["ws"], gscale_dev=gsd, gscale=self.grad_scale)
        K.lw_ratio(lw["ws"], tab, lw["out"], False, group["trust_coef"], group["eps"], group["clamp"], gsd,
                   self.grad_scale)
        K.lars_apply(p, g, buf, _cut(fp.shadow, s, e), tab, lw["out"][:n], group["lr"], group["momentum"],
                     group["dampening"], group["nesterov"], gsd, self.grad_scale, first, hyper=hyper)

    def _step_param(self, group, p, gsd):
        ex = self._excluded(p)
        wd = 0.0 if ex else group["weight_decay"]
        g = self._scaled_grad(p, gsd)
        wn, un = torch.linalg.vector_norm(p), torch.linalg.vector_norm(g)
        r = self._ratio(wn, un, group["trust_coef"] * wn / (un + wd * wn + group["eps"]), not ex, group["clamp"])
        d = (g.add(p, alpha=wd) if wd != 0 else g) * r
        p.add_(self._momentum(group, p, d), alpha=-group["lr"])
        return r, wn, un


class LAMB(_MomentsRule, _LayerwiseBase):
    """Layer-wise adaptive moments (You et al. 2020): Adam's moments m, v of the gradient as the update sees it,

        u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + wd * w;     r = ||w|| / ||u||;     w -= lr * r * u

    per parameter; r = 1 for an excluded parameter (which also gets no weight decay), when ||w|| = 0 or ||u|| = 0;
    ``clamp`` caps r at 1."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, clamp=False,
                 exclude=_exclude_1d):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, clamp=clamp), exclude)

    def _apply_range(self, gi, group, s, e, state, gsd, hyper=None):        # always the group's whole range
        from ..ops import kernels as K
        fp, _ = self._group_flat(gi, group)
        lw = self._lw_prepare(gi, group)
        m, v, t = state
        (b1, b2), eps = group["betas"], group["eps"]
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        tab, n = lw["tab"], lw["tab"].nseg
        p = _cut(fp.data, s, e)
        K.lw_norm_partials(p, _cut(fp.grad, s, e), tab, lw["ws"], m, v, b1, b2, eps, bc1, bc2, gsd, self.grad_scale,
                           hyper=hyper)
        K.lw_ratio(lw["ws"], tab, lw["out"], True, clamp=group["clamp"])
        K.lamb_apply(p, m, v, _cut(fp.shadow, s, e), tab, lw["out"][:n], group["lr"], eps, bc1, bc2, hyper=hyper)

    def _step_param(self, group, p, gsd):
        ex = self._excluded(p)
        wd = 0.0 if ex else group["weight_decay"]
        m, denom, bc1 = self._moments(group, p, self._scaled_grad(p, gsd))
        u = (m / bc1) / denom
        if wd != 0:
            u = u.add(p, alpha=wd)
        wn, un = torch.linalg.vector_norm(p), torch.linalg.vector_norm(u)
        r = self._ratio(wn, un, wn / un, not ex, group["clamp"])
        p.sub_(u * (group["lr"] * r))
        return r, wn, un


__all__ = ["SGD", "Adam", "AdamW", "LARS", "LAMB", "FlatParams"]
