"""ctypes binding of the in-tree HIP kernel library ``_lib/libpdnn_kernels.so``.

The launchers are plain ``extern "C"`` functions taking raw device pointers and a ``hipStream_t``; we
pass ``torch.cuda.current_stream().cuda_stream`` so every kernel is ordered on torch's stream (and is
captured by ``torch.cuda.CUDAGraph`` when a graph capture is active).  The library is loaded after
``import torch`` so it binds to the HIP runtime torch already loaded (same SONAME
``libamdhip64.so.7``) — one runtime, shared streams.

There is deliberately no silent fallback: if a CUDA tensor reaches an op and the library cannot be
loaded, :func:`lib` raises.  CPU tensors never touch this module (the ops use the PyTorch reference
implementation on CPU so the test-suite runs on the GPU-less dev box).
"""
from __future__ import annotations

import ctypes
import functools
import os
from pathlib import Path

import torch

_LIBDIR = Path(__file__).resolve().parent.parent / "_lib"
_LIB = None
_ERR = None

P = ctypes.c_void_p
I = ctypes.c_int
L = ctypes.c_long
F = ctypes.c_float
D = ctypes.c_double

# name -> argtypes (every launcher returns int = hipError_t)
_SIGS = {
    "pdnn_gemm_nt": [P, L, P, L, P, L, I, I, I, F, P, I, I, P],
    "pdnn_gemm_nn": [P, L, P, L, P, L, I, I, I, F, I, P],
    "pdnn_gemm_tn_acc": [P, L, P, L, P, L, I, I, I, F, P],
    "pdnn_conv_fwd": [P, P, P, I, I, I, I, I, I, I, I, I, I, I, P, P, P, P],
    "pdnn_conv_dgrad": [P, P, P, I, I, I, I, I, I, I, I, I, I, I, P, P, P, P, P, P, P, P, P],
    "pdnn_conv_dgrad_stats_rows": [I, I, I, I, I, I, I],
    "pdnn_conv_wgrad": [P, P, P, I, I, I, I, I, I, I, I, I, I, I, P, P, P],
    "pdnn_gemm_stats_rows": [I],
    "pdnn_conv3x3": [P, P, P, I, I, I, I, I, P, P, P, P, P, P, P, P, I, P, P, P, P, P, P, P, P, P, P],
    "pdnn_conv3x3_supported": [I, I, I, I, I],
    "pdnn_conv3x3s2": [P, P, P, I, I, I, I, I, I, P] + [P] * 5 + [P] * 7 + [P, P, I, P],
    "pdnn_conv3x3s2_supported": [I, I, I, I, I],
    "pdnn_conv3x3s2_wgrad": [P, P, P, I, I, I, I, I, P, P, P, P],
    "pdnn_conv3x3s2_wgrad_supported": [I, I, I, I, I],
    "pdnn_conv3x3s2_wgrad_ws": [I, I, I, I, I],
    "pdnn_conv3x3_fp8_supported": [I, I, I, I, I],
    "pdnn_conv3x3_stats_rows": [I, I, I],
    "pdnn_conv3x3_flip": [P, P, I, I, P],
    "pdnn_conv3x3_flip8": [P, P, I, I, P],
    "pdnn_conv3x3_fp8": [P, P, P, I, I, I, I, I, P] + [P] * 5 + [P] * 7 + [P] * 4 + [I, P, P, P],
    "pdnn_conv3x3_wgrad": [P, P, P, I, I, I, I, I, P, P, P, P],
    "pdnn_conv3x3_wgrad_fp8": [P, P, P, I, I, I, I, I, P, P, P, P, P, P, P, P],
    "pdnn_conv3x3_wgrad_supported": [I, I, I, I, I],
    "pdnn_conv3x3_wgrad_ws": [I, I, I, I, I],
    "pdnn_conv3x3_force": [I],
    "pdnn_tune_set": [ctypes.c_char_p, I],
    "pdnn_tune_get": [ctypes.c_char_p],
    "pdnn_tune_list": [ctypes.c_char_p, I],
    "pdnn_tune_error": [],
    "pdnn_tune_unknown": [],
    "pdnn_set_comm_world": [I],
    "pdnn_grid_cus": [],
    "pdnn_conv1x1_panel": [P, P, P, L, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P],
    "pdnn_conv1x1_panel_supported": [L, I, I],
    "pdnn_conv1x1_panel_stats_rows": [L],
    "pdnn_conv1x1_wide": [P, P, P, L, I, I] + [P] * 16,
    "pdnn_conv1x1_wide_supported": [L, I, I],
    "pdnn_stem_conv": [P, P, P, I, I, I, I, I, P, P],
    "pdnn_stem_stats_rows": [L],
    "pdnn_stem_conv_nchw": [P, P, P, I, I, I, I, I, P, P],
    "pdnn_stem_wgrad_nchw": [P, P, P, I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P],
    "pdnn_stem_wgrad_ws": [I, I, I],
    "pdnn_bn_relu_maxpool": [P, P, P, P, P, I, I, I, I, I, I, P],
    "pdnn_set_glds_mode": [I],
    "pdnn_set_pp_mode": [I],
    "pdnn_set_pp_bn": [I],
    "pdnn_set_pp_trace": [P],
    "pdnn_pp_wgrad": [P, L, P, L, P, L, I, I, I, F, P, I, P, I, P],
    "pdnn_pp_wgrad_plan": [I, I, I, I],
    "pdnn_pp_wgrad_splits": [I, I, I],
    "pdnn_pp_wgrad_ws": [I, I, I],
    "pdnn_pp_wgrad_splits_long": [I, I, I],
    "pdnn_pp_gemm_nt_splitk": [P, L, P, L, P, L, I, I, I, P, I, P],
    "pdnn_pp_splitk_splits": [I, I, I],
    "pdnn_transpose_bf16": [P, L, P, L, I, I, P],
    "pdnn_subsample": [P, P, I, I, I, I, I, P],
    "pdnn_transpose_bf16_multi": [P, P, P, P, I, P],
    "pdnn_set_staged_store": [I],
    "pdnn_bn_reduce_rows": [L, I],
    "pdnn_bn_finalize": [P, I, I, D, F, F, P, P, P, P, P, P, P, P, P],
    "pdnn_bn_eval_coeff": [I, F, P, P, P, P, P, P, P],
    "pdnn_bn_stats": [P, L, I, P, P],
    "pdnn_bn_apply": [P, L, I, P, P, P, P, P, I, P, P, P],
    "pdnn_bn_bwd_reduce": [P, P, L, I, P, P, I, P, P, P, P, P, P, P, P, P],
    "pdnn_bn_bwd_finalize": [P, I, I, P, P, I, P, P, P],
    "pdnn_bn_bwd_apply": [P, P, L, I, P, P, P, P, P, I, P, P, P, P, P, P, P, P, P, P, P, P, P],
    "pdnn_maxpool_fwd": [P, P, P, I, I, I, I, I, I, I, I, I, P],
    "pdnn_maxpool_bwd": [P, P, P, I, I, I, I, I, I, I, I, I, P],
    "pdnn_maxpool_bwd_bnred": [P, P, P, P, P, P, P, P, P, I, I, I, I, P],
    "pdnn_maxpool_bwd_bnred_rows": [I, I, I, I],
    "pdnn_stream_wait": [P, P],
    "pdnn_stream_wait_value": [P, P],
    "pdnn_avgpool_fwd": [P, P, I, I, I, P],
    "pdnn_avgpool_bwd": [P, P, I, I, I, P],
    "pdnn_xent_fwd": [P, L, I, I, P, I, P, P, P, P, I, P],
    "pdnn_xent_bwd": [P, L, I, I, P, I, P, P, F, P, P, L, I, P],
    "pdnn_xent_fwd_grad": [P, L, I, I, P, I, P, P, P, P, P, L, P],
    "pdnn_xent_ls_fwd": [P, L, I, I, P, I, F, F, P, P, P, P, I, P],
    "pdnn_xent_ls_bwd": [P, L, I, I, P, I, F, F, P, P, F, P, P, L, I, P],
    "pdnn_xent_ls_fwd_grad": [P, L, I, I, P, I, F, F, P, P, P, P, P, L, P],
    "pdnn_sgd_step": [P, P, P, P, L, F, F, F, F, I, P, F, I, P, P],
    "pdnn_adam_step": [P, P, P, P, P, L, F, F, F, F, F, I, F, F, P, F, P, P],
    "pdnn_cast_f32_bf16": [P, P, L, F, P],
    "pdnn_cast_bf16_f32": [P, P, L, F, I, P],
    "pdnn_scale_f32": [P, L, F, P, I, P],
    "pdnn_axpy_f32": [P, P, L, F, P],
    "pdnn_sumsq_f32": [P, L, P, P],
    "pdnn_sumsq_partials": [P, L, P, I, P],          # returns the number of partials, or -hipError
    "pdnn_clip_coef": [P, I, F, F, P, P, P],
    "pdnn_lw_chunk": [],
    "pdnn_lw_norm_partials": [P, P, P, P, P, P, I, I, P, I, F, F, F, F, F, F, F, P, F, P, P],
    "pdnn_lw_ratio": [P, P, I, I, I, F, F, I, P, F, P, P],
    "pdnn_lars_apply": [P, P, P, P, P, P, I, I, P, F, F, F, I, I, P, F, P, P],
    "pdnn_lamb_apply": [P, P, P, P, P, P, I, I, P, F, F, F, F, P, P],
    "pdnn_act_fwd": [P, P, L, I, P],
    "pdnn_act_bwd": [P, P, P, L, I, P],
    "pdnn_add": [P, P, P, L, F, F, P],
    "pdnn_nchw_to_nhwc": [P, I, P, I, I, I, I, P],
    "pdnn_nhwc_to_nchw_f32": [P, P, I, I, I, I, P],
    "pdnn_colsum": [P, L, I, P, I, P, P],
    "pdnn_colsum_splits": [L],
    "pdnn_gemm_batched": [I, I, I, P, L, L, L, P, L, L, L, P, L, L, L, I, I, I, I, I, F, P, I, P],
    "pdnn_gemm_nt_ex": [P, L, P, L, P, L, I, I, I, F, P, I, P, P, P, I, P],
    "pdnn_gemm_skinny": [P, L, P, P, L, I, I, I, P, I, P, P],
    "pdnn_gemm_skinny_plan": [I, I],
    "pdnn_layernorm_fwd": [P, P, P, P, P, P, I, I, F, P],
    "pdnn_layernorm_bwd_blocks": [I],
    "pdnn_layernorm_bwd": [P, P, P, P, P, P, P, P, I, I, I, P],
    "pdnn_attn_softmax_fwd": [P, L, P, L, P, I, I, F, I, P],
    "pdnn_attn_softmax_bwd": [P, L, P, L, P, L, I, I, F, I, P],
    "pdnn_flash_attn_fwd": [P, P, P, I, I, I, F, I, P, P, F, P, I, P],
    "pdnn_flash_attn_bwd": [P, P, P, P, P, P, I, I, I, F, I, P, P, F, P, I, P],
    "pdnn_doc_bounds": [P, ctypes.c_longlong, P, P, I, I, P],
    "pdnn_attn_decode": [P, P, P, P, P, P, I, I, I, I, F, P],
    "pdnn_attn_decode_ws": [I, I, I, I],
    "pdnn_attn_decode_multi": [P, P, P, P, P, P, I, I, I, I, I, F, P],
    "pdnn_attn_decode_multi_ws": [I, I, I, I, I],
    "pdnn_spec_prepare": [P, I, I, I, P, P, P, ctypes.c_longlong, P, I, I, I, P, P, P, P],
    "pdnn_spec_accept": [P, P, P, I, I, I, P, P, P, ctypes.c_longlong, P, P, I, I, P],
    "pdnn_kv_cache_fill": [P, P, P, I, I, I, I, P],
    "pdnn_kv_cache_append": [P, P, P, P, I, I, I, I, P],
    "pdnn_attn_extend": [P, P, P, P, P, I, I, I, I, F, P],
    "pdnn_attn_extend_tile": [],
    "pdnn_dropout_add_fwd": [P, P, P, L, I, F, P, I, P],
    "pdnn_dropout_bwd": [P, P, L, I, F, P, I, P],
    "pdnn_dropout_mask_rows": [P, L, I, F, P, I, P],
    "pdnn_dropout_mask_attn": [P, I, I, I, F, P, I, P],
    "pdnn_embedding_fwd": [P, P, P, P, I, I, I, P],
    "pdnn_embedding_decode": [P, P, P, P, P, I, I, I, I, P],
    "pdnn_sample_logits": [P, I, L, I, I, F, I, F, P, P, P, P, L, L, P, L, P, P, P],
    "pdnn_embedding_bwd": [P, P, P, P, I, I, I, P],
    "pdnn_embedding_bwd_scaled": [P, P, P, P, I, I, I, F, P],
    "pdnn_gemm_fp8": [P, L, P, L, P, L, I, I, I, P, P, I, P, P, P, I, P],
    "pdnn_fp8_probe": [P, P, P, I, P],
    "pdnn_amax_bf16": [P, L, P, P],
    "pdnn_amax_f32": [P, L, P, P],
    "pdnn_fp8_scale": [P, P, P, I, P],
    "pdnn_fp8_scale_step": [P, P, P, P, P, I, P],
    "pdnn_fp8_scale_roll": [P, P, P, I, I, P],
    "pdnn_quant_fp8": [P, L, P, P, P, P],
    "pdnn_quant_fp8_current": [P, L, P, P, P, I, P],
    "pdnn_quant_fp8_f32": [P, L, P, P, P],
    "pdnn_dequant_fp8": [P, L, P, P, P],
}


def lib_path() -> Path:
    alt = os.environ.get("PDNN_KERNEL_LIB")        # experiments: an alternative build of the same kernels
    return Path(alt) if alt else _LIBDIR / "libpdnn_kernels.so"


def _load():
    global _LIB, _ERR
    if _LIB is not None or _ERR is not None:
        return _LIB
    p = lib_path()
    from .. import _build
    if not p.exists() and os.environ.get("PDNN_AUTOBUILD", "1") == "1":
        try:
            _build.build_kernels()          # under an inter-process lock; objects renamed into place
        except Exception as e:  # pragma: no cover - reported via _ERR
            _ERR = f"could not build {p}: {e}"
            return None
    elif "PDNN_KERNEL_LIB" not in os.environ:
        stale = _build.stale_sources("kernels")
        if stale:
            import warnings
            warnings.warn(f"{p} is older than {len(stale)} kernel source(s) (e.g. {stale[0]}); "
                          "rebuild with `python -m pytorch_distributed_nn_amd._build`", stacklevel=2)
    try:
        lib = ctypes.CDLL(str(p), mode=ctypes.RTLD_GLOBAL)
    except OSError as e:
        _ERR = f"could not load {p}: {e}"
        return None
    for name, argtypes in _SIGS.items():
        fn = getattr(lib, name, None)
        if fn is None:
            continue
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int
    if getattr(lib, "pdnn_dropout_p_eff", None) is not None:     # float -> float, not a launcher
        lib.pdnn_dropout_p_eff.argtypes = [F]
        lib.pdnn_dropout_p_eff.restype = F
    if getattr(lib, "pdnn_tune_error", None) is not None:
        lib.pdnn_tune_error.restype = ctypes.c_char_p
        lib.pdnn_tune_unknown.restype = ctypes.c_char_p
        err = lib.pdnn_tune_error().decode()
        from .. import tuning
        unknown = [k for k in lib.pdnn_tune_unknown().decode().split(",") if k and k not in tuning.DEFAULTS]
        if unknown:
            err += f"PDNN_TUNE: unknown key(s) {unknown}; "
        if err:                  # PDNN_TUNE is malformed or names an entry that exists in neither table: fail loudly
            _ERR = err
            return None
    _LIB = _Lib(lib)
    return _LIB


class _Lib:
    """The CDLL behind a per-name lookup cache.  Pure shape queries (``*_supported``, ``*_rows``, ``*_splits``,
    ``*_ws``, ``*_work``, ``*_blocks``, ``*_groups``: integer arguments -> integer result) are memoised: the
    fused blocks ask several per kernel launch, and at ResNet-50's stage 3-4 the step is bound by the host's
    issue rate (gpurun_out/r4_04: the compute stream idles behind launches).  The memo is cleared whenever a
    dispatch switch changes (clear_query_cache)."""

    _PURE = ("_supported", "_rows", "_splits", "_splits_long", "_ws", "_work", "_blocks", "_groups")

    def __init__(self, cdll):
        self._cdll = cdll
        self._fns = {}

    def __getattr__(self, name):
        f = self._fns.get(name)
        if f is None:
            f = getattr(self._cdll, name)
            if name.endswith(self._PURE):
                f = functools.lru_cache(maxsize=8192)(f)
            elif name.startswith(("pdnn_set_", "pdnn_tune_set")) or name.endswith("_force"):
                f = self._switch(f)              # a dispatch switch: the memoised answers may change
            self._fns[name] = f
            self.__dict__[name] = f              # later lookups bypass __getattr__
        return f

    def _switch(self, raw):
        def call_and_clear(*args):
            r = raw(*args)
            self.clear_query_cache()
            return r
        return call_and_clear

    def clear_query_cache(self):
        for f in self._fns.values():
            if hasattr(f, "cache_clear"):
                f.cache_clear()


def available() -> bool:
    return _load() is not None


def lib():
    """The loaded kernel library; raises (never falls back) if it is unavailable."""
    l = _LIB if _LIB is not None else _load()
    if l is None:
        raise RuntimeError(f"pytorch_distributed_nn_amd: HIP kernel library unavailable ({_ERR}). "
                           "Run `python -m pytorch_distributed_nn_amd._build` (hipcc, gfx950).")
    return l


def clear_query_cache():
    """Forget memoised shape queries (after a dispatch-table or routing switch changed)."""
    if _LIB is not None:
        _LIB.clear_query_cache()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_CUR_DEV = getattr(torch._C, "_cuda_getDevice", None)


def stream(dev=None) -> int:
    """The current HIP stream handle (every launch passes it).  The raw-handle query skips the torch.cuda.Stream
    object torch.cuda.current_stream() builds (dev/probes/host_prims.py)."""
    if dev is None and _RAW_STREAM is not None:
        return _RAW_STREAM(_CUR_DEV())
    return torch.cuda.current_stream(dev).cuda_stream


def ptr(t) -> int | None:
    return None if t is None else t.data_ptr()


class HipError(RuntimeError):
    pass


def call(name: str, *args):
    rc = getattr(_LIB if _LIB is not None else lib(), name)(*args)
    if rc != 0:
        raise HipError(f"{name} failed with hipError {rc}")
    return rc
