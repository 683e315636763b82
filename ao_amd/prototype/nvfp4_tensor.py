"""NVFP4Tensor and the two NVFP4 inference configs (weight-only and dynamic activation), MI355X-native.

Host-side mirror of
  * torchao/prototype/mx_formats/nvfp4_tensor.py:44-50     QuantizeTensorToNVFP4Kwargs
  * torchao/prototype/mx_formats/nvfp4_tensor.py:52-854    NVFP4Tensor (to_nvfp4, dequantize, get_hp_scales, linear / mm / addmm / t / view /
                                                           slice), per_tensor_amax_to_scale, nvfp4_quantize
  * torchao/prototype/mx_formats/inference_workflow.py:173-400  NVFP4DynamicActivationNVFP4WeightConfig, NVFP4WeightOnlyConfig and their
                                                           quantize_ handlers
for bfloat16 weights and activations: e2m1 codes packed two a byte, one float8_e4m3fn scale per 1 x 16 block, an optional fp32 per-tensor
scale.  The cast, the per-tensor amax and both linears run on the HIP kernels of include/ao_mi355.h "NVFP4 linears" (ops.nvfp4_*): the
weight-only linear streams 0.5625 bytes a weight instead of dequantising to bf16 first, and the dynamic linear -- which the reference only
runs on sm100 -- decodes both operands to bf16 in registers, where code x block scale is exact.

Scales are stored ROW-MAJOR [rows, K/16] and `is_swizzled_scales` is always False, for the reason mx_tensor.py gives: the kernels take the
scale bytes as per-lane register operands, so the 128 x 4 blocked layout the reference stores for cuBLAS has no use here.  A scale tensor a
reference run or a checkpoint holds in that layout is un-swizzled once, on load, by NVFP4Tensor.from_reference_layout.  `use_triton_kernel`
is accepted and ignored.  Not implemented (NotImplementedError): float32 weights or activations, 3-D / per-expert weights and
_grouped_mm ON THIS CLASS -- the experts of an MoE layer are an NVFP4ExpertWeights and their GEMM nvfp4_grouped_mm (nvfp4_grouped.py) --
and the observer flow step="prepare" / "convert".
"""
import enum
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..quantization.base_tensor import LowBitTensorBase, aten
from ..quantization.config import AOBaseConfig
from ..quantization.quant_api import register_quantize_module_handler

__all__ = ["NVFP4Tensor", "QuantizeTensorToNVFP4Kwargs", "QuantizationStep", "NVFP4WeightOnlyConfig",
           "NVFP4DynamicActivationNVFP4WeightConfig", "per_tensor_amax_to_scale", "F4_E2M1_MAX", "F8E4M3_MAX"]

# e2m1 code -> value (custom_fp_utils._floatx_unpacked_to_f32(x, 2, 1)); code 8 is -0.0
E2M1_VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
F4_E2M1_MAX = 6.0
F8E4M3_MAX = 448.0
BLOCK = 16


class QuantizationStep(str, enum.Enum):
    """reference quantize_/common/quantization_step.py"""
    PREPARE = "prepare"
    CONVERT = "convert"
    PREPARE_FOR_LOADING = "prepare_for_loading"


@dataclass
class QuantizeTensorToNVFP4Kwargs:
    """reference nvfp4_tensor.py:44-50 (same fields and defaults)"""

    block_size: int = 16
    is_swizzled_scales: bool = False
    use_triton_kernel: bool = False
    use_dynamic_per_tensor_scale: bool = False


def per_tensor_amax_to_scale(amax: torch.Tensor) -> torch.Tensor:
    """reference :756-769"""
    return amax.to(torch.float32) / (F8E4M3_MAX * F4_E2M1_MAX)


def _row_major(qdata):
    return qdata.dim() < 2 or qdata.stride(-2) > qdata.stride(-1)


def _hp_shape(qdata):
    """reference tensor_size_fp4x2_to_hp: two elements a byte along K -- the last dimension of a row-major qdata, the first of its
    transpose."""
    shape = list(qdata.shape)
    shape[-1 if _row_major(qdata) else -2] *= 2
    return shape


def _require_bf16(what, dtype):
    if dtype != torch.bfloat16:
        raise NotImplementedError(f"NVFP4 on MI355X takes bfloat16 {what}, got {dtype}: cast explicitly (.to(torch.bfloat16)) if that "
                                  "rounding is acceptable")


class NVFP4Tensor(LowBitTensorBase):
    """
    Tensor attributes (reference :52-79):
      qdata                 uint8 [N, K/2] packed e2m1 codes, element 2i in the low nibble; the tensor reports [N, K]
      scale                 float8_e4m3fn [N, K/16], row-major (is_swizzled_scales is always False here; see the module docstring)
      per_tensor_scale      fp32 0-dim or None
      act_per_tensor_scale  fp32 0-dim or None: the static per-tensor scale of the activation
    Non-tensor attributes: block_size (16), orig_dtype, is_swizzled_scales, use_triton_kernel, act_quant_kwargs.
    """

    tensor_data_names = ["qdata", "scale"]
    tensor_attribute_names = ["block_size", "orig_dtype"]
    optional_tensor_data_names = ["per_tensor_scale", "act_per_tensor_scale"]
    optional_tensor_attribute_names = ["is_swizzled_scales", "use_triton_kernel", "act_quant_kwargs"]

    def __new__(cls, qdata, scale, block_size, orig_dtype, per_tensor_scale=None, act_per_tensor_scale=None, is_swizzled_scales=False,
                use_triton_kernel=False, act_quant_kwargs=None):
        return torch.Tensor._make_wrapper_subclass(cls, _hp_shape(qdata), dtype=orig_dtype, device=qdata.device, requires_grad=False)

    def __init__(self, qdata, scale, block_size, orig_dtype, per_tensor_scale=None, act_per_tensor_scale=None, is_swizzled_scales=False,
                 use_triton_kernel=False, act_quant_kwargs=None):
        assert qdata.dtype == torch.uint8, f"qdata must be uint8 (packed e2m1 codes), got {qdata.dtype}"
        assert scale.dtype == torch.float8_e4m3fn, f"scale.dtype must be `torch.float8_e4m3fn`, got {scale.dtype}"
        assert not is_swizzled_scales, ("NVFP4Tensor on MI355X stores row-major scales (is_swizzled_scales=False); load a swizzled scale "
                                        "tensor with NVFP4Tensor.from_reference_layout")
        if per_tensor_scale is not None and per_tensor_scale.dim() != 0:
            raise NotImplementedError(f"NVFP4Tensor on MI355X takes a 0-dim per_tensor_scale (per-expert scales belong to "
                                      f"NVFP4ExpertWeights), got shape {tuple(per_tensor_scale.shape)}")
        self.qdata = qdata
        self.scale = scale
        self.block_size = block_size
        self.orig_dtype = orig_dtype
        self.per_tensor_scale = per_tensor_scale
        self.act_per_tensor_scale = act_per_tensor_scale
        self.is_swizzled_scales = is_swizzled_scales
        self.use_triton_kernel = use_triton_kernel
        self.act_quant_kwargs = act_quant_kwargs

    def _quantization_type(self):
        return f"{self.is_swizzled_scales=}, {self.use_triton_kernel=}, {self.act_quant_kwargs=}"

    # the base class rebuilds with (*data, *attributes, **optional data): this class keeps the reference's constructor order
    def _with(self, qdata, scale, per_tensor_scale=None, act_per_tensor_scale=None, orig_dtype=None):
        return NVFP4Tensor(qdata, scale, self.block_size, self.orig_dtype if orig_dtype is None else orig_dtype, per_tensor_scale,
                           act_per_tensor_scale, self.is_swizzled_scales, self.use_triton_kernel, self.act_quant_kwargs)

    def __tensor_flatten__(self):
        return self._data_names(), [self.block_size, self.orig_dtype, self.is_swizzled_scales, self.use_triton_kernel, self.act_quant_kwargs]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        block_size, orig_dtype, swizzled, triton, act_quant_kwargs = tensor_attributes
        return cls(tensor_data_dict["qdata"], tensor_data_dict["scale"], block_size, orig_dtype, tensor_data_dict.get("per_tensor_scale"),
                   tensor_data_dict.get("act_per_tensor_scale"), swizzled, triton, act_quant_kwargs)

    def _apply_fn_to_data(self, fn):
        opt = [fn(t) if t is not None else None for t in (self.per_tensor_scale, self.act_per_tensor_scale)]
        return self._with(fn(self.qdata), fn(self.scale), *opt)

    @staticmethod
    def to_nvfp4(data_hp: torch.Tensor, block_size: int = BLOCK, per_tensor_scale: Optional[torch.Tensor] = None,
                 act_per_tensor_scale: Optional[torch.Tensor] = None, is_swizzled_scales: bool = False, use_triton_kernel: bool = False,
                 act_quant_kwargs: Optional[QuantizeTensorToNVFP4Kwargs] = None):
        """reference :131-194.  The cast runs on the MI355X kernel (ops.nvfp4_quantize: the bytes of the reference's nvfp4_quantize).
        is_swizzled_scales and use_triton_kernel are accepted and ignored: the scales are stored row-major."""
        if data_hp.dim() != 2:
            raise NotImplementedError(f"NVFP4Tensor on MI355X quantizes 2-D tensors (3-D / per-expert weights: "
                                      f"NVFP4ExpertWeights.from_hp), got shape {tuple(data_hp.shape)}")
        _require_bf16("tensors", data_hp.dtype)
        assert block_size == BLOCK, "NVFP4 requires block_size=16"
        assert data_hp.shape[-1] % block_size == 0, "K dim must be divisible by block_size"
        assert data_hp.is_contiguous(), "Only support contiguous data for now"
        from ..torch_ops import kernels

        qdata, scale = kernels(data_hp).nvfp4_quantize(data_hp, per_tensor_scale)
        return NVFP4Tensor(qdata, scale, block_size, data_hp.dtype, per_tensor_scale, act_per_tensor_scale, False, use_triton_kernel,
                           act_quant_kwargs)

    @staticmethod
    def from_reference_layout(qdata: torch.Tensor, swizzled_scale: torch.Tensor, block_size: int = BLOCK, orig_dtype=torch.bfloat16,
                              per_tensor_scale: Optional[torch.Tensor] = None, act_per_tensor_scale: Optional[torch.Tensor] = None,
                              use_triton_kernel: bool = False, act_quant_kwargs: Optional[QuantizeTensorToNVFP4Kwargs] = None):
        """An NVFP4Tensor from the tensors of a reference-produced NVFP4Tensor with is_swizzled_scales=True (or of a checkpoint in that
        layout): qdata [N, K/2] as stored, the scale in to_blocked's 128 x 4 layout (prototype/mx_formats/utils.py:31-72; any shape of
        32 ceil(N / 128) x 16 ceil(K / 64) elements).  The scale is un-swizzled once, here, with plain torch ops: not a hot path."""
        assert qdata.dim() == 2 and qdata.is_contiguous(), "expected a contiguous 2-D qdata [N, K/2]"
        qdata = qdata.view(torch.uint8)
        rows, cols = qdata.shape[0], qdata.shape[1] * 2 // block_size
        rb, cb = (rows + 127) // 128, (cols + 3) // 4
        assert swizzled_scale.numel() == rb * cb * 512, (
            f"a swizzled scale of a [{rows}, {qdata.shape[1] * 2}] tensor has {rb * cb * 512} elements, got {swizzled_scale.numel()}")
        # flat order of the blocked layout: [row block][column block][row % 32][row // 32 % 4][column % 4]
        s = swizzled_scale.contiguous().view(torch.uint8).reshape(rb, cb, 32, 4, 4).permute(0, 3, 2, 1, 4).reshape(rb * 128, cb * 4)
        scale = s[:rows, :cols].contiguous().view(torch.float8_e4m3fn)
        return NVFP4Tensor(qdata, scale, block_size, orig_dtype, per_tensor_scale, act_per_tensor_scale, False, use_triton_kernel,
                           act_quant_kwargs)

    def get_hp_scales(self) -> torch.Tensor:
        """reference :233-257: the block scales in fp32, times the per-tensor scale when there is one (an fp32 product); [N, K/16] of the
        row-major orientation."""
        scale = self.scale if _row_major(self.qdata) else self.scale.transpose(-2, -1)
        s = scale.to(torch.float32)
        return s if self.per_tensor_scale is None else self.per_tensor_scale * s

    def dequantize(self, output_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """reference :199-231: f32(code) times get_hp_scales() in fp32, rounded to the output dtype; the reference's bits."""
        output_dtype = self.dtype if output_dtype is None else output_dtype
        transposed = not _row_major(self.qdata)
        data = self.qdata.transpose(-2, -1) if transposed else self.qdata
        lut = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=data.device)
        codes = torch.stack([data & 0xF, data >> 4], dim=-1).reshape(*data.shape[:-1], data.shape[-1] * 2)
        hp = lut[codes.long()]
        rows, k = hp.shape[-2], hp.shape[-1]
        out = (hp.reshape(rows, k // self.block_size, self.block_size) * self.get_hp_scales().reshape(rows, k // self.block_size, 1))
        out = out.reshape(rows, k).to(output_dtype)
        return out.transpose(-2, -1) if transposed else out


implements = NVFP4Tensor.implements
implements_torch_function = NVFP4Tensor.implements_torch_function


def _transpose(t):
    return t._with(t.qdata.t(), t.scale.t(), t.per_tensor_scale, t.act_per_tensor_scale)


def _as_weight(b):
    """mm / addmm receive the transposed view [K, N] of an [N, K] weight (reference: linear passes weight.t()); the kernels take [N, K]."""
    if not isinstance(b, NVFP4Tensor):
        raise NotImplementedError("NVFP4Tensor: weight must be NVFP4Tensor")
    assert b.qdata.dim() == 2, "expected a 2-D NVFP4Tensor operand"
    return b if _row_major(b.qdata) else _transpose(b)


def _addmm_nvfp4(a, w, bias):
    """reference nvfp4_linear / nvfp4_mm / nvfp4_addmm (:581-706) with w the [N, K] weight and a 2-D."""
    from ..torch_ops import kernels

    if bias is not None and bias.dtype != torch.bfloat16:
        bias = bias.to(torch.bfloat16)
    k = w.act_quant_kwargs
    if isinstance(a, NVFP4Tensor):
        if k is None:  # reference :632-634: both dequantised
            return kernels(a.qdata).nvfp4_wo_linear(a.dequantize(torch.bfloat16).contiguous(), w.qdata, w.scale, w.per_tensor_scale, bias)
        assert _row_major(a.qdata), "the activation must be row-major"
        y = kernels(a.qdata).nvfp4_mm(a.qdata, a.scale, w.qdata, w.scale, a.per_tensor_scale, w.per_tensor_scale, bias)
        return y.to(a.orig_dtype)
    _require_bf16("activations", a.dtype)
    a = a.contiguous()
    if k is None:
        return kernels(a).nvfp4_wo_linear(a, w.qdata, w.scale, w.per_tensor_scale, bias)
    assert k.block_size == BLOCK, f"NVFP4 requires block_size=16, got {k.block_size}"
    if a.shape[0] == 0:
        return a.new_empty((0, w.shape[0]))
    dynamic = bool(k.use_dynamic_per_tensor_scale)
    return kernels(a).nvfp4_linear(a, w.qdata, w.scale, w.per_tensor_scale, None if dynamic else w.act_per_tensor_scale, dynamic, bias)


@implements(aten.linear.default)
@implements_torch_function(F.linear)
def _(func, types, args, kwargs):
    """reference :581-619"""
    a, w = args[0], args[1]
    bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
    if not isinstance(w, NVFP4Tensor):
        raise NotImplementedError("NVFP4Tensor: weight must be NVFP4Tensor")
    a2 = a.view(-1, a.shape[-1]) if isinstance(a, NVFP4Tensor) else a.reshape(-1, a.shape[-1])
    res = _addmm_nvfp4(a2, _as_weight(w), bias)
    return res.reshape(*a.shape[:-1], res.shape[-1])


@implements([aten.mm.default, aten.matmul.default])
@implements_torch_function([torch.mm, torch.matmul])
def _(func, types, args, kwargs):
    """reference :622-652"""
    return _addmm_nvfp4(args[0], _as_weight(args[1]), None)


@implements(aten.addmm.default)
@implements_torch_function(torch.addmm)
def _(func, types, args, kwargs):
    """reference :675-706"""
    assert kwargs.get("alpha", 1) == 1 and kwargs.get("beta", 1) == 1, "only alpha = beta = 1 is supported"
    return _addmm_nvfp4(args[1], _as_weight(args[2]), args[0])


@implements(aten._grouped_mm.default)
def _(func, types, args, kwargs):
    raise NotImplementedError("NVFP4Tensor _grouped_mm (3-D / per-expert weights) is not implemented on MI355X: use "
                              "ao_amd.prototype.nvfp4_grouped_mm on an NVFP4ExpertWeights")


@implements(aten.t.default)
def _(func, types, args, kwargs):
    """reference :403-419"""
    return _transpose(args[0])


@implements(aten.view.default)
def _(func, types, args, kwargs):
    """reference :444-461: the qdata is viewed (the packed dimension halved), the scale kept"""
    t, size = args[0], list(args[1])
    i = -1 if _row_major(t.qdata) else 0
    size[i] = size[i] // 2 if size[i] != -1 else -1
    return t._with(t.qdata.view(size), t.scale, t.per_tensor_scale, t.act_per_tensor_scale)


@implements(aten.slice.Tensor)
def _(func, types, args, kwargs):
    """reference :372-400, rows only: with row-major scales a slice of rows is a slice of both tensors."""
    t, dim = args[0], (args[1] if len(args) > 1 else 0)
    start, end, step = (list(args[2:5]) + [None, None, 1][len(args[2:5]):])
    if step != 1:
        raise ValueError("Only support aten.slice with step=1")
    assert t.qdata.is_contiguous(), "Only support contiguous data for now"
    assert t.qdata.dim() == 2, f"only rank 2 is supported for slice, got rank {t.qdata.dim()}"
    if dim not in (0, -2):
        raise NotImplementedError("NVFP4Tensor on MI355X slices along dim 0 only")
    return t._with(aten.slice.Tensor(t.qdata, 0, start, end, 1), aten.slice.Tensor(t.scale, 0, start, end, 1), t.per_tensor_scale,
                   t.act_per_tensor_scale)


torch.serialization.add_safe_globals([NVFP4Tensor, QuantizeTensorToNVFP4Kwargs, QuantizationStep])


# ---- the configs (inference_workflow.py:173-400) ----------------------------------------------------------------------------------------
@dataclass
class NVFP4DynamicActivationNVFP4WeightConfig(AOBaseConfig):
    """reference inference_workflow.py:173-230 (same fields and defaults).  The weight is cast once, the activation on every call: its
    per-tensor scale from the device amax (use_dynamic_per_tensor_scale) or none.  use_triton_kernel is accepted and ignored; the
    observer flow (step) is not implemented."""

    use_triton_kernel: bool = True
    use_dynamic_per_tensor_scale: bool = True
    step: Optional[QuantizationStep] = None

    def __post_init__(self):
        if isinstance(self.step, str):
            self.step = QuantizationStep(self.step)
        if self.step is not None:
            self.use_dynamic_per_tensor_scale = False  # static quantization implies it


@dataclass
class NVFP4WeightOnlyConfig(AOBaseConfig):
    """reference inference_workflow.py:356-370"""

    use_dynamic_per_tensor_scale: bool = True


def _nvfp4_weight(module, parameter_name):
    weight = getattr(module, parameter_name)
    if weight.dim() < 2 or weight.shape[-2] % 16 != 0 or weight.shape[-1] % 16 != 0:
        raise RuntimeError(f"NVFP4 only supports weight shape with last 2 dims divisible by 16, got {weight.shape}")
    if weight.dim() != 2:
        raise NotImplementedError(f"NVFP4 on MI355X quantizes 2-D weights (3-D / per-expert weights are not implemented), got shape "
                                  f"{tuple(weight.shape)}")
    _require_bf16("weights", weight.dtype)
    return weight.detach().contiguous()


@register_quantize_module_handler(NVFP4DynamicActivationNVFP4WeightConfig)
def _nvfp4_inference_linear_transform(module: nn.Module, config: NVFP4DynamicActivationNVFP4WeightConfig, *, parameter_name: str = "weight"):
    """reference inference_workflow.py:233-353, step=None; no sm100 assert: the GEMM is this library's.  Scales row-major."""
    weight = _nvfp4_weight(module, parameter_name)
    if config.step is not None:
        raise NotImplementedError(f"the NVFP4 observer flow (step={config.step.value!r}) is not implemented on MI355X: pass a static "
                                  "act_per_tensor_scale to NVFP4Tensor.to_nvfp4 instead")
    per_tensor_scale = ops.nvfp4_amax_scale(weight) if config.use_dynamic_per_tensor_scale else None
    act_quant_kwargs = QuantizeTensorToNVFP4Kwargs(use_dynamic_per_tensor_scale=config.use_dynamic_per_tensor_scale,
                                                   use_triton_kernel=config.use_triton_kernel, is_swizzled_scales=False)
    quantized_weight = NVFP4Tensor.to_nvfp4(weight, per_tensor_scale=per_tensor_scale, is_swizzled_scales=False, use_triton_kernel=False,
                                            act_quant_kwargs=act_quant_kwargs)
    quantized_weight.use_triton_kernel = config.use_triton_kernel
    setattr(module, parameter_name, nn.Parameter(quantized_weight, requires_grad=False))
    return module


@register_quantize_module_handler(NVFP4WeightOnlyConfig)
def _nvfp4_weight_only_linear_transform(module: nn.Module, config: NVFP4WeightOnlyConfig, *, parameter_name: str = "weight"):
    """reference inference_workflow.py:373-400"""
    weight = _nvfp4_weight(module, parameter_name)
    per_tensor_scale = ops.nvfp4_amax_scale(weight) if config.use_dynamic_per_tensor_scale else None
    quantized_weight = NVFP4Tensor.to_nvfp4(weight, per_tensor_scale=per_tensor_scale, is_swizzled_scales=False, act_quant_kwargs=None)
    setattr(module, parameter_name, nn.Parameter(quantized_weight, requires_grad=False))
    return module
