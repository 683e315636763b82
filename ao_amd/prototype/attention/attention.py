"""FP8 scaled dot-product attention (mirrors torchao/prototype/attention/shared_utils/attention.py and quantization/quantization.py).

The reference casts with Triton kernels and calls FlashAttention-3 through PyTorch's quantized SDPA, which exists on Hopper only.  Here both
steps are HIP kernels for gfx950: ops.fp8_attn_quantize (one amax launch, one cast launch) and ops.fp8_attn_fwd.

Left out, and refused by name: the Hadamard modes (hadamard != "NONE") and the RoPE-fused entry (_fp8_rope_sdpa)."""
from typing import Optional

import torch

from ao_amd import ops, torch_ops  # noqa: F401  (torch_ops registers ao_mi355::fp8_sdpa)

_BACKEND_NAME = "MI355X"


def _fp8_sdpa_quantize(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor):
    """(q_fp8, k_fp8, v_fp8, descale_q, descale_k, descale_v): per-head FP8 codes [B, H, S, D] and fp32 [B, Hkv] descales, byte for byte the
    reference's triton_fp8_sdpa_quantize.  Strided [B, S, H, D].transpose(1, 2) views are read in place."""
    return ops.fp8_attn_quantize(q, k, v)


def fp8_sdpa(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, attn_mask: Optional[torch.Tensor] = None, dropout_p: float = 0.0,
             is_causal: bool = False, scale: Optional[float] = None, enable_gqa: bool = False, hadamard: str = "NONE") -> torch.Tensor:
    """F.scaled_dot_product_attention's signature on the FP8 path.  Layout [B, H, S, D] in and out; the output has the input dtype.  Grouped
    queries (Hq a multiple of Hkv) are served whether or not enable_gqa is set, as in the reference."""
    if attn_mask is not None:
        raise ValueError(f"attn_mask not supported for FP8 {_BACKEND_NAME}")
    if dropout_p != 0.0:
        raise ValueError(f"dropout_p must be 0.0 for FP8 {_BACKEND_NAME}, got {dropout_p}")
    if hadamard != "NONE":
        raise NotImplementedError(f"hadamard={hadamard!r} is not supported for FP8 {_BACKEND_NAME}: the Hadamard modes are left out")
    return torch.ops.ao_mi355.fp8_sdpa(query, key, value, bool(is_causal), 0.0 if scale is None else float(scale))


def _fp8_rope_sdpa(*args, **kwargs):
    raise NotImplementedError(f"_fp8_rope_sdpa: the RoPE-fused entry is left out of FP8 {_BACKEND_NAME}; apply RoPE, then call fp8_sdpa")
