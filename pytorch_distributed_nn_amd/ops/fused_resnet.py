"""Block-level fused ResNet ops for the GPU path (NHWC bf16 activations, fp32 BN statistics).

A whole Bottleneck / BasicBlock / stem is ONE autograd Function whose forward and backward are
hand-scheduled sequences of HIP kernels (reference modules: pytorch_code/model_ops/resnet.py:14-64;
the reference's layer-wise "Split" backward that streams gradients out early, resnet_split.py:235-326,
is replaced by DDP bucket hooks firing as each block's backward completes).

Fusion plan of a Bottleneck (x -> out):

  forward                                          what is written to HBM
  t1 = conv1x1(x)          + BN1 partial stats      t1
  t2 = conv3x3(relu(bn1(t1)))  + BN2 stats          t2       (BN1 + ReLU applied while the halo kernel stages t1;
                                                            a1 materialised only for the implicit-GEMM routes)
  t3 = conv1x1(relu(bn2(t2)))  + BN3 stats           t3       (a2 never materialised)
  td = conv1x1/s(x)        + BNd stats  (if downsample)
  out = relu(bn3(t3) + bnd(td) | x)   one kernel    out

  backward mirrors it: one reduce + one apply kernel per BN (ReLU masks recomputed from t and the BN
  affine, or read from `out`), conv wgrads read the virtual activations relu(bn(t)) through the same
  fused prologue, dgrads are implicit GEMMs on the weight without any transposed copy.
"""
from __future__ import annotations

from collections import namedtuple
from functools import partial
from itertools import islice
from typing import NamedTuple

import torch

from .. import tuning
from . import kernels as K
from .functional import weight_bf16
from .side_stream import GradSink, prep_weights, side_stream, wait_prepped


class ConvBN(NamedTuple):
    """A conv output t with the state of the BatchNorm that follows it (batch statistics in training, running ones
    in eval) and that BN as an affine: bn(t) = t * scale + shift."""
    t: object
    mean: object
    invstd: object
    scale: object = None
    shift: object = None

    @property
    def pro(self):
        """(scale, shift): the operand prologue of a kernel that reads relu(bn(t)) from t"""
        return self.scale, self.shift

    def stats(self):
        """Without the affine: what a backward that reads its ReLU mask elsewhere keeps"""
        return self._replace(scale=None, shift=None)


_NO_BN = ConvBN(None, None, None)


class _Conv(NamedTuple):
    """One conv + BN of a block: its parameters and, in the forward, running statistics and bf16 weight shadow"""
    w: object
    gamma: object
    beta: object
    rm: object = None
    rv: object = None
    k: object = None


def _convs(n, params, bufs=(), shadows=()):
    """The per-conv groups of a block's flat argument lists (3 parameters, 2 buffers, 1 shadow per conv), padded
    with None to n: a block without a projection shortcut."""
    cs = [_Conv(*params[3 * i:3 * i + 3], *bufs[2 * i:2 * i + 2], *shadows[i:i + 1]) for i in range(len(params) // 3)]
    return cs + [None] * (n - len(cs))


class BlockConf(NamedTuple):
    """conf of BottleneckFn / BasicBlockFn; a plain tuple of the first four fields or more serves too"""
    stride: int
    training: bool
    mom: float
    eps: float
    fp8: object = None          # Fp8Conv2 of a Bottleneck whose conv2 may run on the fp8 halo kernel


def _save(ctx, rec):
    """save_for_backward of a record of tensors and ConvBN fields (flattened; None entries stay None)"""
    ctx.saved_bn = [isinstance(v, ConvBN) for v in rec]
    ctx.save_for_backward(*(t for v, bn in zip(rec, ctx.saved_bn) for t in (v if bn else (v,))))


def _load(ctx, cls):
    it = iter(ctx.saved_tensors)
    return cls(*(ConvBN(*islice(it, 5)) if bn else next(it) for bn in ctx.saved_bn))


def _bn_state(t, slab, c, conf):
    """-> ConvBN of a conv output: training finalizes the conv's statistics slab (and updates the running
    statistics), eval takes the coefficients of the running ones."""
    if conf.training:
        M = t.numel() // t.shape[-1]
        return ConvBN(t, *K.bn_finalize(slab, slab.shape[0] // 2, M, conf.eps, conf.mom, c.gamma, c.beta, c.rm, c.rv))
    sc, sh = K.bn_eval_coeff(conf.eps, c.gamma, c.beta, c.rm, c.rv)
    return ConvBN(t, c.rm, torch.rsqrt(c.rv + conf.eps), sc, sh)


def _conv_bn(x, c, st, pad, pro, conf):
    t, slab = K.conv_fwd(x, c.k, st, pad, pro=pro, want_stats=conf.training)
    return _bn_state(t, slab, c, conf)


def _act(a, bn):
    """-> (input, operand prologue) of a kernel that reads relu(bn(t)): the materialised a, else t with BN + ReLU"""
    return (a, None) if a is not None else (bn.t, bn.pro)


class _Sink(GradSink):
    """Parameter-gradient routing of one fused backward (GradSink), with its kernels.

    Weight gradients run on a side HIP stream: a conv's wgrad (dt, x -> dW) and the data-gradient chain
    (dt -> dgrad -> BN backward -> next dt) are independent, so the split-K wgrad blocks fill the partial
    last rounds of the dgrad grids (and vice versa) instead of each kernel draining the chip on its own.
    Each wgrad is ordered after everything queued on the compute stream so far (its operands); `done()`
    joins the side stream back before the gradients are announced.  The operands stay referenced by the
    block's backward until that join, so the caching allocator cannot hand their memory out early; a
    hipGraph capture records the fork/join as graph edges."""

    def __init__(self, device=None):
        super().__init__(side_stream(device) if device is not None else None)

    def bn(self, slab, rows, p):
        """-> (dgamma, dbeta) for bn_bwd_apply, (returned grads of gamma, beta)"""
        acc = self.acc(p.gamma, p.beta)
        dg, db = K.bn_bwd_finalize(slab, rows, acc=acc)
        return (dg, db), ((None, None) if acc is not None else (dg, db))

    def wgrad(self, w_p, x, dy, R, S, st, pad, pro=None, fp8=None):
        if self.side is None:
            return self._wgrad(w_p, x, dy, R, S, st, pad, pro, fp8)
        return self._fork(w_p, x, dy, R, S, st, pad, pro, fp8)

    def _fork(self, w_p, x, dy, R, S, st, pad, pro, fp8):
        # (holding a weight gradient back to share the next fork's marker measured neutral: run r3_60)
        main = torch.cuda.current_stream(x.device)
        self.fork(main)
        with torch.cuda.stream(self.side):
            g = self._wgrad(w_p, x, dy, R, S, st, pad, pro, fp8)
        # the side stream may still read the operands after this block's backward returned (deferred join):
        # the caching allocator must not hand their memory to the compute stream before that work is done
        for t in (x, dy) + (tuple(pro) if pro is not None else ()):
            t.record_stream(self.side)
        if g is not None:
            g.record_stream(main)        # allocated on the side stream, consumed by autograd on the main one
            self.returned = True
        return g

    def _wgrad(self, w_p, x, dy, R, S, st, pad, pro, fp8=None):
        acc = self.acc(w_p)
        if fp8 is not None:          # fp8 conv2 (Fp8Conv2): both operands' scales are current for x and dy
            if acc is not None:
                K.conv3x3_wgrad_fp8(x, dy, fp8.fwd, fp8.bwd, out=acc[0].permute(0, 2, 3, 1), pro=pro)
                return None
            return _krsc_grad(K.conv3x3_wgrad_fp8(x, dy, fp8.fwd, fp8.bwd, pro=pro))
        if acc is not None:
            K.conv_wgrad(x, dy, R, S, st, pad, pro=pro, out=acc[0].permute(0, 2, 3, 1))
            return None
        return _krsc_grad(K.conv_wgrad(x, dy, R, S, st, pad, pro=pro))


def _conv3x3_bn_fp8(a1, c, act, conf, pro=None):
    """conv2 (3x3, stride 1) forward on the fp8 halo kernel: a1 quantised to e4m3 in the kernel's halo staging
    (delayed scaling, no separate quantisation pass), e4m3 weight (current scaling, once per weight version),
    fused BN statistics."""
    from .fp8 import weight_fp8
    wq, winv = weight_fp8(c.w, krsc=True)
    t, slab = K.conv3x3_fp8(a1, wq, winv, act, want_stats=conf.training, pro=pro)
    return _bn_state(t, slab, c, conf)


class Fp8Conv2:
    """fp8 state of one Bottleneck's 3x3 conv (BASELINE.json config 5): the forward operand a1 in e4m3, the data
    gradient's operand dt2 in e5m2, each with its own delayed scale."""

    def __init__(self, device):
        from .fp8 import Fp8Act
        self.fwd = Fp8Act(device)
        self.bwd = Fp8Act(device, e5m2=True)


def _shortcut_fwd(x, cd, conf):
    """The projection shortcut conv + BN statistics -> (ConvBN of td, its input).  Stride 2 (tuning ds_sub): the
    conv reads a contiguous copy of x's even pixels, so it runs as a stride-1 1x1 conv and its
    weight gradient as a plain GEMM (the implicit-GEMM engine's strided gathers ran the ResNet-50 shortcut forwards at
    7-10% and their weight gradients at 5-13% of the bf16 peak: 0.86 + 1.04 ms per step, r5_52 trace)."""
    if conf.stride > 1 and tuning.get("ds_sub") and x.shape[-1] % 8 == 0:
        xs = K.subsample(x, conf.stride)
        return _conv_bn(xs, cd, 1, 0, None, conf), xs
    return _conv_bn(x, cd, conf.stride, 0, None, conf), x


def _bn_apply0(gm, bn, gamma, dgamma, dbeta):
    """dt of a BN whose masked gradient gm and sums are known: the apply pass on its own"""
    C = bn.t.shape[-1]
    dt, _, _ = K.bn_bwd_apply(gm.view(-1, C), bn.t.view(-1, C), bn.mean, bn.invstd, gamma, dgamma, dbeta, mode=0)
    return dt.view(bn.t.shape)


def _pre(bn, gamma, dgamma, dbeta):
    """The same apply as the operand prologue of the next data gradient (K.conv_dgrad pre=), which also writes dt
    (the last entry) for the weight gradient"""
    return (bn.t, bn.mean, bn.invstd, gamma, dgamma, dbeta, torch.empty_like(bn.t))


def _bn_back(g2d, t2d, bn, gamma, mode, sink, p, msrc=None, msc=None, msh=None):
    slab, _, rows = K.bn_bwd_reduce(g2d, t2d, bn.mean, bn.invstd, mode=mode, msrc=msrc, mscale=msc, mshift=msh)
    (dgamma, dbeta), ret = sink.bn(slab, rows, p)
    dt, _, _ = K.bn_bwd_apply(g2d, t2d, bn.mean, bn.invstd, gamma, dgamma, dbeta, mode=mode, msrc=msrc, mscale=msc,
                              mshift=msh)
    return dt, ret


def _out_bn_back(sink, gout, mb, bn, p, gamma, bnd, pd, gammad):
    """The block-output BN's backward, with the shortcut BN's (bnd, pd, gammad) when there is one, under the ReLU
    mask of `out` -> dt, dtd or None, returned grads of (gamma, beta), of the shortcut's.  Without a shortcut BN the
    identity branch's gradient gout * mask is added by conv1's data gradient (res_mask) rather than materialised
    here: one activation-sized write less per block (+0.2%, run r3_07)."""
    C = bn.t.shape[-1]
    g2d, t2d = gout.view(-1, C), bn.t.view(-1, C)
    td2d = bnd.t.view(-1, C) if pd is not None else None
    slab, slabd, rows = K.bn_bwd_reduce(g2d, t2d, bn.mean, bn.invstd, mode=3, msrc=mb, x2=td2d, mean2=bnd.mean,
                                        invstd2=bnd.invstd)
    (dg, db), ret = sink.bn(slab, rows, p)
    (dgd, dbd), retd = sink.bn(slabd, rows, pd) if pd is not None else ((None, None), (None, None))
    dt, dtd, _ = K.bn_bwd_apply(g2d, t2d, bn.mean, bn.invstd, gamma, dg, db, mode=3, msrc=mb, x2=td2d, mean2=bnd.mean,
                                invstd2=bnd.invstd, gamma2=gammad, dgamma2=dgd, dbeta2=dbd)
    return dt.view(bn.t.shape), dtd.view(bnd.t.shape) if pd is not None else None, ret, retd


def _prep_dgrad_weights(x, specs):
    """Make the data gradients' transformed weights (K.dgrad_weight: flipped 3x3, transposed 1x1) in the
    forward, on the side stream, which is idle there: the backward then finds them ready instead of running
    ~30 small transform kernels on its critical path.  specs: [(dy_shape, w, x_shape, st, pad) or None].
    -> side_stream.prep_weights' result"""
    return prep_weights(x.device, [(sp[1], partial(K.dgrad_weight, *sp)) if sp is not None else None for sp in specs])


def _pre_ok(t, wk, st, pad):
    """Whether the consumer of dt = bn_bwd_apply(gm, t) (data gradient of the conv with weight wk) takes the
    apply as its operand prologue."""
    return K.dgrad_pre_ok(tuple(t.shape), tuple(wk.shape), st, pad)


def _dgrad_bn_gm(dy, wk, bn, st, pad, sink, p, wprep=None):
    """dgrad whose epilogue applies the ReLU mask of relu(bn(t)) and reduces the BN-backward sums, stopped before
    the apply pass: -> (gm, dgamma, dbeta, returned grads).  The apply then runs inside the next data gradient's
    operand loads (_pre)."""
    gm, slab = K.conv_dgrad(dy, wk, bn.t.shape, st, pad, bn=bn, wprep=wprep)
    (dgamma, dbeta), ret = sink.bn(slab, slab.shape[0] // 2, p)
    return gm, dgamma, dbeta, ret


def _fused_dgrad_bn(dy, wk, bn, st, pad, gamma, sink, p, wprep=None):
    """_dgrad_bn_gm, then one apply pass produces dt (the gradient w.r.t. the BN input t) -> dt, returned grads"""
    gm, dgamma, dbeta, ret = _dgrad_bn_gm(dy, wk, bn, st, pad, sink, p, wprep=wprep)
    return _bn_apply0(gm, bn, gamma, dgamma, dbeta), ret


def _input_grads(sink, s, gout, p1, geo1, dy1, pre1, pd, dtd, stride, w1p=None):
    """The tail of a block's backward -> dx, dw1, dwd: conv1's weight gradient (before everything else when dt1 = dy1
    exists, after conv1's data gradient when that one writes it: pre1), the shortcut's weight gradient, conv1's data
    gradient and the shortcut branch.  geo1 = conv1's (kernel size, stride, pad); s: the saved record."""
    R, st, pad = geo1
    dwd = None
    if pre1 is None:
        dw1 = sink.wgrad(p1.w, s.x, dy1, R, R, st, pad)
    if pd is not None:
        # (with the subsampled input the shortcut's weight gradient is a plain GEMM: dtd^T . xs)
        dwd = (sink.wgrad(pd.w, s.xs, dtd, 1, 1, 1, 0) if s.xs is not None
               else sink.wgrad(pd.w, s.x, dtd, 1, 1, stride, 0))
        dx = K.conv_dgrad(dy1, s.k1, s.x.shape, st, pad, pre=pre1, wprep=w1p)
        # shortcut branch accumulated in place: a stride-2 1x1 dgrad only touches the pixels its taps
        # reach, so no zero-filled full-size buffer and no extra full read/write pass
        dx = K.conv_dgrad(dtd, s.kd, s.x.shape, stride, 0, res=dx, out=dx)
    else:
        # the identity branch: gout * mask added by conv1's data-gradient epilogue (_out_bn_back)
        dx = K.conv_dgrad(dy1, s.k1, s.x.shape, st, pad, res=gout.view(s.x.shape), res_mask=s.mb, pre=pre1, wprep=w1p)
    if pre1 is not None:
        dw1 = sink.wgrad(p1.w, s.x, pre1[-1], R, R, st, pad)       # dt1 written by conv1's data gradient
    return dx, dw1, dwd


def _krsc_grad(dw):
    """fp32 [K][R][S][C] -> [K][C][R][S] view with channels_last strides (the parameter's layout)."""
    return dw.permute(0, 3, 1, 2)


_BottleneckSaved = namedtuple("_BottleneckSaved", "x a1 a2 xs mb b1 b2 b3 bd g1 g2 g3 gd k1 k2 k3 kd")
_BasicBlockSaved = namedtuple("_BasicBlockSaved", "x a1 xs mb b1 b2 bd g1 g2 gd k1 k2 kd")
_StemSaved = namedtuple("_StemSaved", "x mb idx bn gamma")


class BottleneckFn(torch.autograd.Function):
    """Bottleneck (expansion 4): params = (w1,g1,b1, w2,g2,b2, w3,g3,b3[, wd,gd,bd])."""

    @staticmethod
    def forward(ctx, x, conf, bufs, shadows, *params):
        conf = BlockConf(*conf)
        stride, training = conf.stride, conf.training
        c1, c2, c3, cd = _convs(4, params, bufs, shadows)
        down = cd is not None
        side_down = None
        xd = x                           # the shortcut conv's input (x, or its stride-2 subsample)
        side = side_stream(x.device) if down else None
        if side is not None:
            # the shortcut conv only depends on x: run it (and its BN statistics) beside conv1 -> conv2 -> conv3
            main = torch.cuda.current_stream(x.device)
            K.stream_wait(side, main)
            with torch.cuda.stream(side):
                side_down, xd = _shortcut_fwd(x, cd, conf)
            x.record_stream(side)
            for t in side_down + (xd,):
                t.record_stream(main)
        b1 = _conv_bn(x, c1, 1, 0, None, conf)
        t1 = b1.t
        C1, K2 = t1.shape[-1], c2.w.shape[0]
        if stride == 1 and K.conv3x3_pro_ok(tuple(t1.shape), K2):
            # a1 = relu(bn1(t1)) is never materialised: the halo conv and the direct weight gradient apply BN1 + ReLU
            # while staging t1 (each element staged ~1.2x: one read of t1 instead of a bn_apply pass writing a1;
            # +0.2% ResNet-50 / +0.3% ResNet-152 same box, run r4_52)
            a1, pro1, src1 = None, b1.pro, t1
        elif stride == 2 and K.conv3x3s2_a1_ok(tuple(t1.shape), K2) and not (
                conf.fp8 is not None and K.conv3x3_fp8_ok(*t1.shape, K2)):
            # stride 2 (tuning s2_halo bit 64): the half-resolution halo conv applies BN1 + ReLU while staging t1's
            # parity planes and writes the result as a1 for the weight gradient -- no separate bn_apply pass
            a1, pro1, src1 = torch.empty_like(t1), b1.pro, t1
        elif stride == 2 and K.conv3x3s2_fold_ok(tuple(t1.shape), K2):
            # stride 2 (tuning s2_halo bit 4): the half-resolution halo conv applies BN1 + ReLU while staging each
            # parity plane of t1, the weight gradient through its operand prologue
            a1, pro1, src1 = None, b1.pro, t1
        else:
            # the implicit-GEMM engine gathers every element 9 times: materialise a1 once instead
            a1 = K.bn_apply(t1.view(-1, C1), b1.scale, b1.shift, relu=True).view(t1.shape)
            pro1, src1 = None, a1
        fp8 = conf.fp8 if (conf.fp8 is not None and stride == 1 and K.conv3x3_fp8_ok(*t1.shape, K2)) else None
        if fp8 is not None:
            b2 = _conv3x3_bn_fp8(src1, c2, fp8.fwd, conf, pro=pro1)
        elif a1 is not None and pro1 is not None:      # a1 written by the stride-2 forward (bit 64 above)
            b2 = _bn_state(*K.conv3x3s2(t1, c2.k, want_stats=training, pro=pro1, pro_out=a1), c2, conf)
        else:
            b2 = _conv_bn(src1, c2, stride, 1, pro1, conf)
        # a2 = relu(bn2(t2)): on the A-stationary 1x1 kernel conv3 applies BN2 + ReLU to its activation fragments
        # once per pixel tile as they are loaded (and its weight gradient in the implicit-GEMM engine's operand
        # prologue), so a2 is never written (tuning a2_fold); elsewhere it is written once -- the 128-row engine's
        # prologue re-ran the affine for every 64-column output tile (run r3_03: 2.82 ms/step vs 0.29 +
        # 1.87 materialised)
        t2 = b2.t
        C2 = t2.shape[-1]
        fold = tuning.get("a2_fold")
        P2 = t2.numel() // C2
        a2 = None
        if not (fold and K.conv1x1_pro_ok(tuple(t2.shape), c3.k.shape[0]) and (fold == 2 or P2 > K.WGRAD1X1_PP_PIX)):
            a2 = K.bn_apply(t2.view(-1, C2), b2.scale, b2.shift, relu=True).view(t2.shape)
        src2, pro2 = _act(a2, b2)
        b3 = _conv_bn(src2, c3, 1, 0, pro2, conf)
        t3 = b3.t
        C3 = t3.shape[-1]
        bd = _NO_BN
        if down:
            if side_down is not None:
                K.stream_wait(main, side)
                bd = side_down
            else:
                bd, xd = _shortcut_fwd(x, cd, conf)
        # (a projection shortcut: the residual is bnd(td), else x itself -- rscale = rshift = None)
        out, mb = K.bn_apply(t3.view(-1, C3), b3.scale, b3.shift, res=(bd.t if down else x).view(-1, C3), rscale=bd.scale,
                             rshift=bd.shift, relu=True, want_mask=training)
        out = out.view(t3.shape)
        ctx.wprep = None
        if training:
            # (an fp8 conv2 takes its flipped e4m3 weight from ops.fp8.weight_fp8_flip instead)
            ctx.wprep = _prep_dgrad_weights(x, [(tuple(t3.shape), c3.k, tuple(t2.shape), 1, 0),
                                                (tuple(t2.shape), c2.k, tuple(t1.shape), stride, 1) if fp8 is None
                                                else None,
                                                (tuple(t1.shape), c1.k, tuple(x.shape), 1, 0)])
        # backward needs only the ReLU mask of `out`: 1 bit per element (mask mode 3), not the bf16 tensor
        _save(ctx, _BottleneckSaved(x, a1, a2, xd if (down and xd is not x) else None, mb, b1, b2, b3.stats(), bd.stats(),
                                    c1.gamma, c2.gamma, c3.gamma, cd.gamma if down else None,
                                    c1.k, c2.k, c3.k, cd.k if down else None))
        ctx.conf = conf
        ctx.params = params
        ctx.fp8 = fp8
        return out

    @staticmethod
    def backward(ctx, gout):
        s = _load(ctx, _BottleneckSaved)
        stride = ctx.conf.stride
        if not ctx.conf.training:
            raise RuntimeError("fused Bottleneck backward requires training-mode BatchNorm")
        gout = gout.contiguous()
        p1, p2, p3, pd = _convs(4, ctx.params)
        ctx.params = None
        sink = _Sink(gout.device)
        w3p = w2p = w1p = None
        if ctx.wprep is not None:
            (w3p, w2p, w1p), ticket = ctx.wprep
            wait_prepped(gout.device, ticket)
            ctx.wprep = None
        # block output BN3 (+BNd) with the ReLU mask of `out`
        dt3, dtd, r3, rd = _out_bn_back(sink, gout, s.mb, s.b3, p3, s.g3, s.bd, pd, s.gd)
        # conv3 (input a2 = relu(bn2(t2)), or t2 with BN2 + ReLU as the operand prologue when a2 was folded)
        x3, pro3 = _act(s.a2, s.b2)
        dw3 = sink.wgrad(p3.w, x3, dt3, 1, 1, 1, 0, pro=pro3)
        x2, pro2 = _act(s.a1, s.b1)
        if _pre_ok(s.b2.t, s.k2, stride, 1):
            # BN2's apply runs in conv2's data-gradient operand loads, which also write dt2 for the wgrad
            gm2, dg2, db2, r2 = _dgrad_bn_gm(dt3, s.k3, s.b2, 1, 0, sink, p2, wprep=w3p)
            pre2 = _pre(s.b2, s.g2, dg2, db2)
            if ctx.fp8 is not None:
                # fp8 data gradient: dt2 (applied in the halo staging) quantised to e5m2 there, tap-flipped e4m3 weight
                from .fp8 import weight_fp8_flip
                wt8, winv = weight_fp8_flip(p2.w)
                gm1, slab1 = K.conv3x3_fp8(gm2, wt8, winv, ctx.fp8.bwd, bn=s.b1, pre=pre2)
            else:
                gm1, slab1 = K.conv_dgrad(gm2, s.k2, s.b1.t.shape, stride, 1, bn=s.b1, pre=pre2, wprep=w2p)
            del gm2
            dw2 = sink.wgrad(p2.w, x2, pre2[-1], 3, 3, stride, 1, pro=pro2, fp8=ctx.fp8)
        else:
            dt2, r2 = _fused_dgrad_bn(dt3, s.k3, s.b2, 1, 0, s.g2, sink, p2, wprep=w3p)
            dw2 = sink.wgrad(p2.w, x2, dt2, 3, 3, stride, 1, pro=pro2)
            gm1, slab1 = K.conv_dgrad(dt2, s.k2, s.b1.t.shape, stride, 1, bn=s.b1, wprep=w2p)
        (dg1, db1), r1 = sink.bn(slab1, slab1.shape[0] // 2, p1)
        if _pre_ok(s.b1.t, s.k1, 1, 0):
            pre1, dy1 = _pre(s.b1, s.g1, dg1, db1), gm1
        else:
            pre1, dy1 = None, _bn_apply0(gm1, s.b1, s.g1, dg1, db1)
        dx, dw1, dwd = _input_grads(sink, s, gout, p1, (1, 1, 0), dy1, pre1, pd, dtd, stride, w1p)
        sink.done()
        return (dx, None, None, None, dw1, *r1, dw2, *r2, dw3, *r3) + ((dwd, *rd) if pd is not None else ())


class BasicBlockFn(torch.autograd.Function):
    """BasicBlock (expansion 1): params = (w1,g1,b1, w2,g2,b2[, wd,gd,bd])."""

    @staticmethod
    def forward(ctx, x, conf, bufs, shadows, *params):
        conf = BlockConf(*conf)
        c1, c2, cd = _convs(3, params, bufs, shadows)
        down = cd is not None
        b1 = _conv_bn(x, c1, conf.stride, 1, None, conf)
        C1 = b1.t.shape[-1]
        a1 = K.bn_apply(b1.t.view(-1, C1), b1.scale, b1.shift, relu=True).view(b1.t.shape)    # 3x3 consumer: materialise
        b2 = _conv_bn(a1, c2, 1, 1, None, conf)
        C2 = b2.t.shape[-1]
        bd, xd = _shortcut_fwd(x, cd, conf) if down else (_NO_BN, x)
        out, mb = K.bn_apply(b2.t.view(-1, C2), b2.scale, b2.shift, res=(bd.t if down else x).view(-1, C2),
                             rscale=bd.scale, rshift=bd.shift, relu=True, want_mask=conf.training)
        out = out.view(b2.t.shape)
        _save(ctx, _BasicBlockSaved(x, a1, xd if xd is not x else None, mb, b1, b2.stats(), bd.stats(), c1.gamma, c2.gamma,
                                    cd.gamma if down else None, c1.k, c2.k, cd.k if down else None))
        ctx.conf = conf
        ctx.params = params
        return out

    @staticmethod
    def backward(ctx, gout):
        s = _load(ctx, _BasicBlockSaved)
        stride = ctx.conf.stride
        if not ctx.conf.training:
            raise RuntimeError("fused BasicBlock backward requires training-mode BatchNorm")
        gout = gout.contiguous()
        p1, p2, pd = _convs(3, ctx.params)
        ctx.params = None
        sink = _Sink(gout.device)
        dt2, dtd, r2, rd = _out_bn_back(sink, gout, s.mb, s.b2, p2, s.g2, s.bd, pd, s.gd)
        dw2 = sink.wgrad(p2.w, s.a1, dt2, 3, 3, 1, 1)
        if _pre_ok(s.b1.t, s.k1, stride, 1):
            # BN1's apply inside conv1's data-gradient operand loads (dt1 written there for the wgrad)
            dy1, dg1, db1, r1 = _dgrad_bn_gm(dt2, s.k2, s.b1, 1, 1, sink, p1)
            pre1 = _pre(s.b1, s.g1, dg1, db1)
        else:
            dy1, r1 = _fused_dgrad_bn(dt2, s.k2, s.b1, 1, 1, s.g1, sink, p1)
            pre1 = None
        dx, dw1, dwd = _input_grads(sink, s, gout, p1, (3, stride, 1), dy1, pre1, pd, dtd, stride)
        sink.done()
        return (dx, None, None, None, dw1, *r1, dw2, *r2) + ((dwd, *rd) if pd is not None else ())


class StemFn(torch.autograd.Function):
    """conv(k, stride, pad) -> BN -> ReLU [-> maxpool(3, 2, 1)] on a channel-padded NHWC input.

    params = (w, gamma, beta); the weight shadow is zero-padded to the input's channel count."""

    @staticmethod
    def forward(ctx, x, conf, bufs, shadows, w, gamma, beta):
        stride, pad, pool, training, mom, eps = conf
        conf = BlockConf(stride, training, mom, eps)
        c = _Conv(w, gamma, beta, *bufs, shadows[0])
        kpad = c.k
        nchw = kpad.dim() == 3          # shadow from K.stem_weight_nchw: x is the NCHW bf16 batch itself
        direct = nchw or (pool and K.stem_ok(x.shape, kpad.shape, stride, pad))
        if direct:
            # direct 7x7/s2 kernel, then BN + ReLU + max-pool in one pass over t; the backward recomputes the
            # ReLU mask from t (mask mode 2), so neither the activation nor its mask is stored.  NCHW: the weight
            # gradient reads the NCHW batch itself too (stem_wgrad.hip): no NHWC copy at all
            stem_conv = K.stem_conv_nchw if nchw else K.stem_conv
            bn = _bn_state(*stem_conv(x, kpad, want_stats=training), c, conf)
            y, idx = K.bn_relu_maxpool(bn.t, bn.scale, bn.shift)
            mb = None
        else:
            bn = _conv_bn(x, c, stride, pad, None, conf)
            C = bn.t.shape[-1]
            a, mb = K.bn_apply(bn.t.view(-1, C), bn.scale, bn.shift, relu=True, want_mask=training)
            a = a.view(bn.t.shape)
            if pool:
                y, idx = K.maxpool_fwd(a, 3, 2, 1)
            else:
                y, idx = a, None
        _save(ctx, _StemSaved(x, mb, idx, bn if direct else bn.stats(), gamma))
        ctx.nchw_wgrad = nchw
        ctx.conf = (stride, pad, pool, w.shape, (w.shape[0], 7, 7, 8) if nchw else kpad.shape)
        ctx.params = (w, gamma, beta)
        return y

    @staticmethod
    def backward(ctx, gy):
        s = _load(ctx, _StemSaved)
        t, bn = s.bn.t, s.bn
        stride, pad, pool, wshape, kshape = ctx.conf
        gy = gy.contiguous()
        C = t.shape[-1]
        p = _Conv(*ctx.params)
        ctx.params = None
        sink = _Sink()
        if ctx.nchw_wgrad and s.mb is None:
            # the BN backward's apply runs inside the NCHW weight-gradient kernel's staging: dt never written;
            # its statistics come out of the max-pool gather's pass
            fused = K.maxpool_bwd_bnred(gy, s.idx, t, bn.mean, bn.invstd, bn.scale, bn.shift) if pool else None
            if fused is not None:
                ga, slab, rows = fused
            else:
                ga = K.maxpool_bwd(gy, s.idx, t.shape, 3, 2, 1) if pool else gy
                slab, _, rows = K.bn_bwd_reduce(ga.view(-1, C), t.view(-1, C), bn.mean, bn.invstd, mode=2,
                                               msrc=t.view(-1, C), mscale=bn.scale, mshift=bn.shift)
            (dg_, db_), (dg, db) = sink.bn(slab, rows, p)
            pre = (t, bn.mean, bn.invstd, s.gamma, dg_, db_, bn.scale, bn.shift)
            acc = sink.acc(p.w)
            if acc is not None and acc[0].stride() == (147, 1, 21, 3):
                K.stem_wgrad_nchw(s.x, ga, pre=pre, acc=acc[0])       # added straight into the arena
                dw = None
            else:
                dw = K.stem_wgrad_nchw(s.x, ga, pre=pre)
                if acc is not None:
                    acc[0].add_(dw)
                    dw = None
            sink.done()
            return None, None, None, None, dw, dg, db
        ga = K.maxpool_bwd(gy, s.idx, t.shape, 3, 2, 1) if pool else gy
        # direct stem: ReLU mask recomputed from t (t * s + h > 0); else the stored mask (no scale / shift saved)
        mode, msrc = (2, t.view(-1, C)) if s.mb is None else (3, s.mb)
        dt, (dg, db) = _bn_back(ga.view(-1, C), t.view(-1, C), bn, s.gamma, mode, sink, p, msrc=msrc, msc=bn.scale,
                                msh=bn.shift)
        dt = dt.view(t.shape)
        if kshape[3] == wshape[1]:
            dw = sink.wgrad(p.w, s.x, dt, kshape[1], kshape[2], stride, pad)
        else:
            dwk = K.conv_wgrad(s.x, dt, kshape[1], kshape[2], stride, pad)     # [K][R][S][Cpad]
            dw = dwk[:, :, :, : wshape[1]].permute(0, 3, 1, 2)
        sink.done()
        # the stem input is the data batch: no input gradient is produced
        return None, None, None, None, dw, dg, db


def stem_shadow(w, cpad):
    """bf16 [K][R][S][Cpad] weight for a channel-padded stem input."""
    k = weight_bf16(w, krsc=True)
    if k.shape[-1] != cpad:
        k = torch.nn.functional.pad(k, (0, cpad - k.shape[-1])).contiguous()
    return k
