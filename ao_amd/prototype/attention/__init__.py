"""Low-precision attention (torchao/prototype/attention) on the MI355X: per-head FP8 casts of Q / K / V and an FP8 flash-attention forward,
both hand-written for gfx950 (csrc/attention_kernels.hip)."""
from .api import AttentionBackend, HadamardMode, apply_low_precision_attention  # noqa: F401
from .attention import _fp8_rope_sdpa, _fp8_sdpa_quantize, fp8_sdpa  # noqa: F401

__all__ = ["AttentionBackend", "HadamardMode", "apply_low_precision_attention", "fp8_sdpa", "_fp8_sdpa_quantize"]
