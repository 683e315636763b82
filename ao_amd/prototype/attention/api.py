"""User-facing API for low-precision attention (mirrors torchao/prototype/attention/api.py)."""
from enum import Enum
from typing import Optional

import torch
import torch._dynamo
import torch.nn as nn

from .attention import fp8_sdpa
from .wrapper import _FP8AttentionMonkeyPatchWrapper, _LowPrecisionAttentionWrapper


class HadamardMode(str, Enum):
    """Hadamard transform mode.  Only NONE is built here; QKV and V_ONLY are refused by name."""

    NONE = "NONE"
    QKV = "QKV"
    V_ONLY = "V_ONLY"


class AttentionBackend(str, Enum):
    """Backend kernel for computing attention."""

    FP8_FA3 = "FP8_FA3"  # the reference's: Hopper plus the flash-attn package; refused here
    FP8_MI355X = "FP8_MI355X"  # the gfx950 kernels of this package; what backend=None resolves to


def apply_low_precision_attention(model: nn.Module, backend: Optional[AttentionBackend] = None,
                                  hadamard: HadamardMode = HadamardMode.NONE) -> nn.Module:
    """Wrap `model` so that every F.scaled_dot_product_attention call inside its forward runs the FP8 path (per-head FP8 casts of Q / K / V,
    then the FP8 flash attention).  Call before torch.compile, with KV caching off.  Returns the wrapper."""
    if isinstance(model, _LowPrecisionAttentionWrapper):
        raise RuntimeError("apply_low_precision_attention has already been applied to this module.")
    if isinstance(model, torch._dynamo.OptimizedModule):
        raise RuntimeError("apply_low_precision_attention must be called before torch.compile.")
    if backend is None:
        backend = AttentionBackend.FP8_MI355X
    if backend == AttentionBackend.FP8_FA3:
        raise RuntimeError("FP8_FA3 requires Hopper (SM 9.x) and the flash-attn package; on the MI355X use AttentionBackend.FP8_MI355X.")
    if backend != AttentionBackend.FP8_MI355X:
        raise ValueError(f"Unknown backend: {backend}")
    if HadamardMode(hadamard) != HadamardMode.NONE:
        raise NotImplementedError(f"HadamardMode.{HadamardMode(hadamard).name} is not supported by the FP8_MI355X backend: the Hadamard modes "
                                  "and the RoPE-fused entry are left out")
    return _FP8AttentionMonkeyPatchWrapper(model, sdpa_patch_fn=fp8_sdpa)
