"""GPTQ for MI355X: GPTQConfig and gptq_quantize.

Host-side mirror of torchao/prototype/gptq/api.py (same public names, same two-step flow):

    quantize_(model, GPTQConfig(step="observe", base_config=...))   # weights become GPTQObserverTensor
    for batch in calibration: model(batch)                          # every F.linear folds its input into the Hessian
    quantize_(model, GPTQConfig(step="convert", base_config=...))   # weights become Int4Tensor / Int8Tensor / NVFP4Tensor

The reference's convert step is launch-bound: for every column of the weight it runs about a dozen eager ops on [N, 1] slices
(api.py:502-526).  Here the whole column loop of one GPTQ block is ONE launch (ops.gptq_block, csrc/gptq_kernels.hip, which states the
arithmetic), and the lazy batch update of the columns right of the block (:530-532) one torch matmul; the dead-column handling, the damping
and the three Cholesky calls (:392-403) are torch ops on the device.  Nothing in the loop synchronises.

Deviation, on purpose: the int8 per-row scale is Int8Tensor's, over the WHOLE row of the original weight, taken once before
block 0; the reference takes it from the first GPTQ block's columns only, because its G_k_end is clipped to the block (:458, :471-478).

Not implemented, refused by name: 3-D expert weights (gptq_quantize_3d), int4 packing formats other than PLAIN, the HQQ qparams, the
fp8-activation (symmetric) int4 flavour, int8 granularities other than PerRow, NVFP4 without the dynamic per-tensor scale, weights that are
neither bfloat16 nor float32.
"""
from dataclasses import dataclass

import torch
import torch.nn as nn

from ... import ops
from ...quantization.config import (
    AOBaseConfig,
    Float8DynamicActivationInt4WeightConfig,
    Int4ChooseQParamsAlgorithm,
    Int4PackingFormat,
    Int4WeightOnlyConfig,
    Int8WeightOnlyConfig,
)
from ...quantization.granularity import PerRow
from ...quantization.quant_api import _set_weight_only, register_quantize_module_handler
from ..nvfp4_tensor import NVFP4DynamicActivationNVFP4WeightConfig, NVFP4Tensor, QuantizeTensorToNVFP4Kwargs
from .observer import GPTQObserverTensor

__all__ = ["GPTQConfig", "gptq_quantize", "gptq_quantize_3d"]


@dataclass
class GPTQConfig(AOBaseConfig):
    """reference api.py:63-103 (same fields and defaults).

    step: "observe" wraps the weight as GPTQObserverTensor; "convert" quantizes it with the Hessian it collected.
    base_config: Int4WeightOnlyConfig (PLAIN), Int8WeightOnlyConfig(granularity=PerRow()) or
        NVFP4DynamicActivationNVFP4WeightConfig(use_dynamic_per_tensor_scale=True): the format of the result.
    percdamp: damping of the Hessian's diagonal.  gptq_quantize_block_size: columns of one GPTQ block, a multiple of the group size, at
    most 256 (ops.GPTQ_MAX_BLOCK: the block's tile lives in LDS)."""

    step: str = "observe"
    base_config: AOBaseConfig = None
    percdamp: float = 0.01
    gptq_quantize_block_size: int = 256

    def __post_init__(self):
        if self.base_config is None:
            raise ValueError("base_config is required for GPTQ quantization.")


def _format_of(base_config):
    """(ops format, group size) of a supported base_config; everything else is refused by name."""
    if isinstance(base_config, Float8DynamicActivationInt4WeightConfig):
        raise NotImplementedError("GPTQ on MI355X: the fp8-activation (symmetric) int4 flavour (Float8DynamicActivationInt4WeightConfig) is not "
                                  "implemented; the column loop is the zero-point flavour of Int4WeightOnlyConfig (prototype/gptq/api.py:167-221)")
    if isinstance(base_config, Int4WeightOnlyConfig):
        if base_config.int4_packing_format != Int4PackingFormat.PLAIN:
            raise NotImplementedError(f"GPTQ on MI355X produces Int4Tensor (int4_packing_format PLAIN) only, got "
                                      f"{base_config.int4_packing_format.value!r}")
        if base_config.int4_choose_qparams_algorithm == Int4ChooseQParamsAlgorithm.HQQ:
            raise NotImplementedError("GPTQ on MI355X: the HQQ qparams algorithm is not implemented; GPTQ freezes min / max (tinygemm) group "
                                      "qparams")
        return ops.GPTQ_INT4, base_config.group_size
    if isinstance(base_config, Int8WeightOnlyConfig):
        if not isinstance(base_config.granularity, PerRow) or base_config.granularity.dim != -1:
            raise NotImplementedError(f"GPTQ only supports per-row int8 quantization (PerRow()), got {base_config.granularity}")
        return ops.GPTQ_INT8, 0
    if isinstance(base_config, NVFP4DynamicActivationNVFP4WeightConfig):
        if not base_config.use_dynamic_per_tensor_scale:
            raise NotImplementedError("GPTQ on MI355X: NVFP4 without the dynamic per-tensor scale (use_dynamic_per_tensor_scale=False, or a "
                                      "static step) is not implemented, as in the reference (api.py:374)")
        return ops.GPTQ_NVFP4, 16
    raise NotImplementedError(f"GPTQ on MI355X: unsupported base_config {type(base_config).__name__}; use Int4WeightOnlyConfig, "
                              "Int8WeightOnlyConfig or NVFP4DynamicActivationNVFP4WeightConfig")


def _check_weight(W):
    if W.dim() == 3:
        raise NotImplementedError("GPTQ on MI355X: 3-D expert weights (gptq_quantize_3d) are not implemented")
    if W.dim() != 2:
        raise NotImplementedError(f"GPTQ quantizes 2-D weights, got shape {tuple(W.shape)}")
    if W.dtype not in (torch.bfloat16, torch.float32):
        raise NotImplementedError(f"GPTQ on MI355X takes bfloat16 or float32 weights, got {W.dtype}")


def _int8_row_scale(W):
    """Int8Tensor.from_hp(W, PerRow()).scale as fp32 [N]: amax / 127.5 in the weight's dtype, clamped at fp32 eps (int8_tensor.py:198-211).
    bf16: the cast kernel's own scale.  fp32 (Int8Tensor.from_hp takes bf16 only): torch ops, the divisor a TENSOR -- torch divides a
    device tensor by a Python scalar as a multiplication by its reciprocal, which is not the correctly rounded quotient."""
    if W.dtype == torch.bfloat16:
        return ops.int8_quantize_rowwise(W)[1].reshape(-1)
    amax = W.abs().amax(dim=1)
    return torch.clamp(amax / torch.full_like(amax, 127.5), min=torch.finfo(torch.float32).eps)


def _nvfp4_per_tensor_scale(W):
    """per_tensor_amax_to_scale(max |W|) (nvfp4_tensor.py:756-769) as one fp32 on the device: amax / 2688, correctly rounded (as above)."""
    if W.dtype == torch.bfloat16:
        return ops.nvfp4_amax_scale(W)
    return torch.max(torch.abs(W)) / torch.tensor(2688.0, dtype=torch.float32, device=W.device)


def gptq_quantize(H: torch.Tensor, W_t: torch.Tensor, config: GPTQConfig):
    """GPTQ (https://arxiv.org/abs/2210.17323, Algorithm 1) as the reference's gptq_quantize (api.py:311-597) runs it: the weight is
    quantized column by column, every column's error spread over the columns not yet quantized, so that ||X W - X W'|| is minimised.

    H: the Hessian [K, K] fp32 (GPTQObserverTensor.hessian); W_t: the weight [N, K], bfloat16 or float32, contiguous; both on the GPU.
    Like the reference this CONSUMES both: H is damped in place and W_t is the working matrix (it ends as the propagated weight whose
    round-to-nearest codes are the result).  Returns an Int4Tensor (compute layout built), an Int8Tensor, or an NVFP4Tensor with the fields
    of NVFP4DynamicActivationNVFP4WeightConfig(use_dynamic_per_tensor_scale=True) weights (row-major scales)."""
    fmt, group_size = _format_of(config.base_config)
    _check_weight(W_t)
    B = int(config.gptq_quantize_block_size)
    W = W_t.detach()
    if not W.is_contiguous():
        raise RuntimeError("gptq_quantize: W_t must be contiguous (it is the working matrix, updated in place)")
    n, k = W.shape
    # the shape rules of ao_gptq_block, all of them, HERE: a refusal from the entry would come after H and W have been changed in place.
    # With K and B multiples of the group size and of 16, so is every block's start and the short last block's width.
    if n == 0 or k == 0:
        raise ValueError(f"gptq_quantize: empty weight of shape {tuple(W.shape)}")
    if fmt == ops.GPTQ_INT4 and group_size not in (32, 64, 128, 256):
        raise ValueError(f"gptq_quantize: int4 group_size must be one of 32, 64, 128, 256, got {group_size}")
    g = group_size if fmt != ops.GPTQ_INT8 else 16  # int8 has no group: the kernel's 16-byte steps
    if k % g != 0 or k % 16 != 0:
        raise ValueError(f"gptq_quantize: K={k} must be a multiple of the group size {g} and of 16")
    if B <= 0 or B % g != 0 or B % 16 != 0:
        raise ValueError(f"gptq_quantize: gptq_quantize_block_size={B} must be a positive multiple of the group size {g} and of 16")
    if B > ops.GPTQ_MAX_BLOCK:
        raise ValueError(f"gptq_quantize: gptq_quantize_block_size={B} is larger than {ops.GPTQ_MAX_BLOCK}, the most one launch holds in LDS")
    if not W.is_cuda:
        raise RuntimeError(f"gptq_quantize: expected the weight on the GPU, got {W.device} (the MI355X backend has no CPU fallback)")
    if H.dtype != torch.float32 or tuple(H.shape) != (k, k) or H.device != W.device:
        raise RuntimeError(f"gptq_quantize: H must be a float32 [{k}, {k}] tensor on {W.device}")
    dev = W.device

    # what is measured on the ORIGINAL weight, before the dead columns go (api.py:379-380 for NVFP4)
    kw = {}
    if fmt == ops.GPTQ_INT4:
        qdata = torch.empty((n, k // 2), dtype=torch.uint8, device=dev)
        kw = dict(group_size=group_size, scale=torch.empty((k // group_size, n), dtype=W.dtype, device=dev),
                  zero_point=torch.empty((k // group_size, n), dtype=W.dtype, device=dev))
    elif fmt == ops.GPTQ_INT8:
        row_scale = _int8_row_scale(W)
        qdata = torch.empty((n, k), dtype=torch.int8, device=dev)
        kw = dict(row_scale=row_scale)
    else:
        p = _nvfp4_per_tensor_scale(W)
        qdata = torch.empty((n, k // 2), dtype=torch.uint8, device=dev)
        kw = dict(scale=torch.empty((n, k // 16), dtype=torch.uint8, device=dev), per_tensor_scale=p)

    # api.py:392-403
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    W[:, dead] = 0
    damp = config.percdamp * torch.mean(torch.diag(H))
    diag = torch.arange(k, device=dev)
    H[diag, diag] += damp
    H = torch.linalg.cholesky(H)
    H = torch.cholesky_inverse(H)
    Hinv = torch.linalg.cholesky(H, upper=True).contiguous()

    for k0 in range(0, k, B):
        end = min(k0 + B, k)
        err = ops.gptq_block(W, Hinv, k0, end - k0, fmt, qdata, **kw)
        if end < k:  # lazy batch update (:530-532): fp32 matmul, rounded into W's dtype by the in-place op
            W[:, end:] -= err.matmul(Hinv[k0:end, end:])

    if fmt == ops.GPTQ_INT4:
        from ...quantization.int4_plain_tensor import Int4Tensor

        out = Int4Tensor(qdata, kw["scale"], kw["zero_point"], [1, group_size], W.shape, act_pre_scale=None)
        out.tile_packed()
        return out
    if fmt == ops.GPTQ_INT8:
        from ...quantization.int8_tensor import Int8Tensor

        return Int8Tensor(qdata, kw["row_scale"].reshape(n, 1), [1, k], W.dtype)
    base = config.base_config
    act_quant_kwargs = QuantizeTensorToNVFP4Kwargs(use_dynamic_per_tensor_scale=base.use_dynamic_per_tensor_scale,
                                                   use_triton_kernel=base.use_triton_kernel, is_swizzled_scales=False)
    return NVFP4Tensor(qdata, kw["scale"].view(torch.float8_e4m3fn), 16, W.dtype, per_tensor_scale=kw["per_tensor_scale"],
                       act_per_tensor_scale=None, is_swizzled_scales=False, use_triton_kernel=base.use_triton_kernel,
                       act_quant_kwargs=act_quant_kwargs)


def gptq_quantize_3d(H: torch.Tensor, W_t: torch.Tensor, config: GPTQConfig):
    """reference api.py:600-640 (MoE expert weights): not implemented."""
    raise NotImplementedError("GPTQ on MI355X: 3-D expert weights (gptq_quantize_3d) are not implemented")


@register_quantize_module_handler(GPTQConfig)
def _gptq_config_transform(module: nn.Module, config: GPTQConfig, *, parameter_name="weight") -> nn.Module:
    """reference api.py:111-164"""
    tensor = getattr(module, parameter_name)
    if config.step == "observe":
        _format_of(config.base_config)  # an unsupported target is refused before any calibration is spent on it
        _check_weight(tensor)
        return _set_weight_only(module, parameter_name, GPTQObserverTensor.from_hp(tensor.detach()))
    if config.step == "convert":
        if not isinstance(tensor, GPTQObserverTensor):
            raise ValueError(f"Expected {parameter_name} to be GPTQObserverTensor in 'convert' step, but got {type(tensor)}. "
                             "Did you run the 'observe' step first?")
        if tensor.batches == 0:
            raise ValueError(f"No observations recorded for {parameter_name}. total_batches is 0. "
                             "Did you run forward passes during the observe step?")
        new_tensor = gptq_quantize(tensor.hessian, tensor.hp_data, config)
        return _set_weight_only(module, parameter_name, new_tensor)
    raise ValueError(f"Invalid step '{config.step}'. Must be 'observe' or 'convert'.")
