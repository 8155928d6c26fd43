"""Fused flat-buffer optimizers (single-launch SGD / Adam / AdamW, layer-wise LARS / LAMB) and the parameter arena."""
from .flat import FlatParams, flatten_module  # noqa: F401
from .fused import LAMB, LARS, SGD, Adam, AdamW  # noqa: F401
