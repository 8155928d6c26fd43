"""The weight-gradient side stream: one HIP stream per device beside the compute stream, and the fork / join
bookkeeping of everything that runs on it (the fused ResNet blocks' and GPT-2 blocks' weight gradients, the
ResNet forward's shortcut convs and data-gradient weight transforms, fp8 / transposed weight prefetches).

:class:`GradSink` is the parameter-gradient routing that the fused backwards share: arena targets, the announce
list and the one rule that decides when the side stream is joined back (:func:`join_now`)."""
from __future__ import annotations

import contextlib

import torch

from .. import tuning
from ..optim.flat import SHADOW_EPOCH, direct_grad, grad_ready
from . import kernels as K

_SIDE = {}        # device index -> stream
_FORKS = {}       # device index -> weight-gradient forks issued so far
_JOINED = {}      # device index -> forks covered by the last end-of-backward join
_FWD_FORKED = {}      # device index -> flat.SHADOW_EPOCH when the side stream last waited on the compute stream
                      # in this model forward (a later mid-forward shadow re-cast needs a new fork)
_WPREP_SEQ = [0]      # weight-prep events in issue order
_WPREP_WAITED = {}    # device index -> highest weight-prep sequence number the compute stream has waited on


def side_stream_if_active(t):
    """The side stream that may still be writing weight gradients of `t`'s device, else None."""
    return _SIDE.get(t.device.index) if t.is_cuda else None


def side_stream(dev):
    """The weight-gradient side stream of a device (tuning side_wgrad = 0 disables it).  It runs at the
    default (lowest) priority; the compute stream gets the high one (bench.py)."""
    if not tuning.get("side_wgrad") or dev.type != "cuda":
        return None
    s = _SIDE.get(dev.index)
    if s is None:
        s = _SIDE[dev.index] = torch.cuda.Stream(device=dev, priority=0)
    return s


def fork_counts(dev):
    """-> (weight-gradient forks issued on the device so far, forks covered by its last end-of-backward join)"""
    return _FORKS.get(dev.index, 0), _JOINED.get(dev.index, 0)


def join_at_backward_end(side):
    # one callback per block (not a shared "already queued" flag, which an aborted backward would leave set);
    # the first to run joins every fork issued so far, the rest find nothing new and add no marker (the
    # callbacks all run after the last backward node, so the first join covers them all; one join per block
    # instead: -0.3%, run r3_60).  A final callback runs with backward()'s caller stream current (the
    # stream the optimizer step follows on: tools/callback_stream_probe.py, run r3_64)
    dev = side.device.index

    def join():
        n = _FORKS.get(dev, 0)
        if _JOINED.get(dev) == n:
            return
        K.stream_wait(torch.cuda.current_stream(side.device), side)
        _JOINED[dev] = n
    torch.autograd.Variable._execution_engine.queue_callback(join)


def join_now(returned, ready):
    """The join rule of a backward that forked weight gradients onto the side stream.  True: they are consumed
    now (returned to autograd, or read on the compute stream by a grad-ready hook of a ``ready`` parameter), so
    the compute stream joins before they are announced.  False: nothing reads them before the optimizer
    (side-aware hooks, i.e. DDP's bucket launches, order their collectives after the side stream themselves:
    side_stream_if_active), so one join at the end of the backward serves, and a block's last weight gradients
    also overlap the next block's data-gradient chain."""
    return returned or not all(getattr(fn, "_pdnn_side_aware", False)
                               for p in ready for fn in getattr(p, "_pdnn_grad_hooks", ()))


class GradSink:
    """Parameter-gradient routing of one fused backward: gradients go straight into the flat arena
    (optim.flat.direct_grad) when possible -- the op then returns None for them and announces them with
    grad_ready in :meth:`done` -- otherwise they are returned to autograd.  A subclass issues the kernels; one
    that runs them on the side stream calls :meth:`fork` first and sets ``returned`` when it hands a gradient made
    there back to autograd."""

    def __init__(self, side=None):
        self.ready = []
        self.side = side
        self.forked = False
        self.returned = False

    def target(self, p):
        """The arena gradient of one parameter (announced by done()), else None"""
        t = direct_grad(p)
        if t is not None:
            self.ready.append(p)
        return t

    def acc(self, *ps):
        """The arena gradients of all of ``ps``, or None (and nothing announced) if any has none"""
        tg = [direct_grad(p) for p in ps]
        if any(t is None for t in tg):
            return None
        self.ready += ps
        return tg

    def fork(self, main):
        """The side stream waits for everything queued on ``main`` so far (the operands of what follows)"""
        K.stream_wait(self.side, main)
        self.forked = True
        _FORKS[main.device.index] = _FORKS.get(main.device.index, 0) + 1

    def done(self):
        if self.forked:
            self.forked = False
            if join_now(self.returned, self.ready):
                K.stream_wait(torch.cuda.current_stream(self.side.device), self.side)
            else:
                join_at_backward_end(self.side)
        for p in self.ready:
            grad_ready(p)


@contextlib.contextmanager
def side_forward(dev):
    """Around a model's block loop: the side stream waits on the compute stream ONCE (the optimizer step that
    refreshed the weights is then behind it), so the blocks' weight transforms need no fork of their own (one
    fork per block: 10,819-10,821 vs 10,844-10,853 img/s, run r3_73)."""
    side = side_stream(dev)
    if side is None:
        yield
        return
    K.stream_wait(side, torch.cuda.current_stream(dev))
    _FWD_FORKED[dev.index] = SHADOW_EPOCH[0]
    try:
        yield
    finally:
        _FWD_FORKED.pop(dev.index, None)


def prep_weights(dev, jobs):
    """Make transformed weights in the forward, on the side stream, which is idle there.  jobs: [(weight, make) or
    None], ``make()`` -> the transformed weight or None.  -> (list of make()'s results, ticket for wait_prepped),
    or None without a side stream."""
    side = side_stream(dev)
    if side is None:
        return None
    main = torch.cuda.current_stream(dev)
    if _FWD_FORKED.get(dev.index) != SHADOW_EPOCH[0]:
        # no fork in this forward yet, or a shadow slice was re-cast on the compute stream since the last one
        # (a PS weight bucket that landed mid-forward): the transforms must read the fresh weights
        K.stream_wait(side, main)
        if dev.index in _FWD_FORKED:
            _FWD_FORKED[dev.index] = SHADOW_EPOCH[0]
    with torch.cuda.stream(side):
        ws = [j[1]() if j is not None else None for j in jobs]
        ev = torch.cuda.Event()
        ev.record(side)
    for j, w in zip(jobs, ws):
        if j is None:
            continue
        j[0].record_stream(side)
        if w is not None:
            w.record_stream(main)
    _WPREP_SEQ[0] += 1
    return ws, (ev, _WPREP_SEQ[0])


def wait_prepped(dev, ticket):
    """The backward's wait for its block's transformed weights.  The side stream is in order, so waiting on the
    latest prep event covers every earlier one: only the first block of the backward (the last of the forward)
    waits."""
    ev, seq = ticket
    if _WPREP_WAITED.get(dev.index, -1) >= seq:
        return
    torch.cuda.current_stream(dev).wait_event(ev)
    _WPREP_WAITED[dev.index] = max(seq, _WPREP_WAITED.get(dev.index, -1))
