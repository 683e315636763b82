"""MXTensor and the MX inference config (MXFP8 / MXFP4 dense linears), MI355X-native.

Host-side mirror of
  * torchao/prototype/mx_formats/mx_tensor.py:100-109   QuantizeTensorToMXKwargs
  * torchao/prototype/mx_formats/mx_tensor.py:508-940   MXTensor (to_mx, dequantize, mm / addmm / linear / t / view)
  * torchao/prototype/mx_formats/inference_workflow.py:80-171  MXDynamicActivationMXWeightConfig and its quantize_ handler
for e4m3 (MXFP8) and e2m1 (MXFP4) elements with block 32.  KernelPreference.AUTO / TORCH run the HIP kernels (ops.mx_linear: the 1 x 32
cast of the activation and the scaled-MFMA GEMM, include/ao_mi355.h "MX dense linears"); EMULATED does what the reference does:
dequantise both operands, then aten mm / addmm.

Scales are stored ROW-MAJOR [rows, K/32] and `is_swizzled_scales` is always False: CDNA4's scaled MFMA takes the E8M0 bytes as per-lane
register operands, so the 128 x 4 blocked layout the reference's transform stores for cuBLAS (for a 48 x 128 weight a [32, 16] scale
tensor) has no use here.  A weight quantized here therefore has a [48, 4] scale tensor.
"""
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..quantization.base_tensor import LowBitTensorBase, aten
from ..quantization.config import AOBaseConfig, KernelPreference
from ..quantization.quant_api import register_quantize_module_handler
from .mx import BLOCK, ScaleCalculationMode

__all__ = ["MXTensor", "QuantizeTensorToMXKwargs", "MXDynamicActivationMXWeightConfig", "E2M1_VALUES"]

_ELEM_DTYPES = (torch.float8_e4m3fn, torch.float4_e2m1fn_x2)

# e2m1 code -> value (custom_fp_utils._floatx_unpacked_to_f32(x, 2, 1)); code 8 is -0.0
E2M1_VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def _validate_elem_dtype(elem_dtype):
    if elem_dtype not in _ELEM_DTYPES:
        raise NotImplementedError(f"MX on MI355X implements float8_e4m3fn and float4_e2m1fn_x2 elements, got {elem_dtype}")


@dataclass
class QuantizeTensorToMXKwargs:
    """reference mx_tensor.py:100-109 (same fields and defaults)"""

    elem_dtype: object = torch.float8_e4m3fn
    block_size: int = 32
    scaling_mode: ScaleCalculationMode = ScaleCalculationMode.FLOOR
    kernel_preference: KernelPreference = KernelPreference.EMULATED
    is_swizzled_scales: bool = False


def _hp_shape(qdata, elem_dtype):
    """The high-precision shape an MXTensor reports: fp4 packs two elements a byte along K (the last dimension of a row-major qdata, the
    first of its transpose) -- reference tensor_size_fp4x2_to_hp."""
    shape = list(qdata.shape)
    if elem_dtype == torch.float4_e2m1fn_x2:
        if qdata.dim() < 2 or qdata.is_contiguous():
            shape[-1] *= 2
        else:
            shape[-2] *= 2
    return shape


class MXTensor(LowBitTensorBase):
    """
    Tensor attributes (reference :508-560):
      qdata  float8_e4m3fn [N, K] (MXFP8) or uint8 [N, K/2] packed e2m1 codes, element 2i in the low nibble (MXFP4); the tensor reports
             [N, K] either way
      scale  float8_e8m0fnu [N, K/32], row-major (is_swizzled_scales is always False here; see the module docstring)
    Non-tensor attributes: elem_dtype, block_size (32), orig_dtype, kernel_preference, act_quant_kwargs, is_swizzled_scales.
    """

    tensor_data_names = ["qdata", "scale"]
    tensor_attribute_names = ["elem_dtype", "block_size", "orig_dtype", "kernel_preference", "act_quant_kwargs", "is_swizzled_scales"]

    def __new__(cls, qdata, scale, elem_dtype, block_size, orig_dtype, kernel_preference, act_quant_kwargs, is_swizzled_scales):
        return torch.Tensor._make_wrapper_subclass(cls, _hp_shape(qdata, elem_dtype), dtype=orig_dtype, device=qdata.device,
                                                   requires_grad=False)

    def __init__(self, qdata, scale, elem_dtype, block_size, orig_dtype, kernel_preference, act_quant_kwargs, is_swizzled_scales):
        if elem_dtype == torch.float8_e4m3fn:
            assert qdata.dtype == elem_dtype, f"qdata.dtype must match elem_dtype for MXFP8 tensors, got {qdata.dtype=} and {elem_dtype=}"
        assert scale.dtype == torch.float8_e8m0fnu, f"scale.dtype must be `torch.float8_e8m0fnu`, got {scale.dtype}"
        assert qdata.dtype in (torch.float8_e4m3fn, torch.uint8), "unsupported"
        assert not is_swizzled_scales, "MXTensor on MI355X stores row-major scales (is_swizzled_scales=False)"
        self.qdata = qdata
        self.scale = scale
        self.elem_dtype = elem_dtype
        self.block_size = block_size
        self.orig_dtype = orig_dtype
        self.kernel_preference = kernel_preference
        self.act_quant_kwargs = act_quant_kwargs
        self.is_swizzled_scales = is_swizzled_scales

    def _quantization_type(self):
        return (f"elem_dtype={self.elem_dtype}, block_size={self.block_size}, orig_dtype={self.orig_dtype}, "
                f"kernel_preference={self.kernel_preference}, act_quant_kwargs={self.act_quant_kwargs}")

    def _with(self, qdata, scale):
        return MXTensor(qdata, scale, self.elem_dtype, self.block_size, self.orig_dtype, self.kernel_preference, self.act_quant_kwargs,
                        self.is_swizzled_scales)

    @staticmethod
    def to_mx(data_hp: torch.Tensor, elem_dtype, block_size: int = BLOCK, scaling_mode: ScaleCalculationMode = ScaleCalculationMode.FLOOR,
              kernel_preference: KernelPreference = KernelPreference.EMULATED, act_quant_kwargs: Optional[QuantizeTensorToMXKwargs] = None,
              is_swizzled_scales: bool = False):
        """reference :630-690.  The cast runs on the MI355X kernels (ops.mxfp8_quantize / ops.mxfp4_quantize, the bytes of the reference's
        to_mx).  is_swizzled_scales is accepted and ignored: the scales are stored row-major."""
        _validate_elem_dtype(elem_dtype)
        if block_size != BLOCK:
            raise NotImplementedError(f"MXTensor on MI355X implements block_size 32 only, got {block_size}")
        assert data_hp.dtype == torch.bfloat16, f"{data_hp.dtype} is not supported yet (bfloat16 only on MI355X)"
        assert data_hp.shape[-1] % block_size == 0, (
            f"the last dimension of shape {data_hp.shape} must be divisible by block_size {block_size}")
        assert data_hp.is_contiguous(), "unsupported"
        qdata, scale = ops.mx_quantize(data_hp, ops.mx_fmt(elem_dtype), scaling_mode)
        return MXTensor(qdata, scale, elem_dtype, block_size, data_hp.dtype, kernel_preference, act_quant_kwargs, False)

    def dequantize(self, output_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """reference :412-471, :600-628: element -> output dtype, times 2^(scale - 127) in the output dtype (NaN where the scale byte is
        255); the reference's bits."""
        output_dtype = self.dtype if output_dtype is None else output_dtype
        data, scale = self.qdata, self.scale
        transposed = data.dim() == 2 and not data.is_contiguous()
        if transposed:
            data, scale = data.t(), scale.t()
        if self.elem_dtype == torch.float4_e2m1fn_x2:
            lut = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=data.device)
            codes = torch.stack([data & 0xF, data >> 4], dim=-1).reshape(*data.shape[:-1], data.shape[-1] * 2)
            hp = lut[codes.long()].to(output_dtype)
        else:
            hp = data.to(output_dtype)
        s = scale.view(torch.uint8)
        s_fp = torch.pow(torch.full(s.shape, 2.0, dtype=torch.float32, device=s.device), s.to(torch.int16) - 127)
        s_fp = torch.where(s != 255, s_fp, float("nan")).to(output_dtype)
        out = (hp.reshape(-1, self.block_size) * s_fp.reshape(-1, 1)).reshape(hp.shape)
        return out.t() if transposed else out


implements = MXTensor.implements
implements_torch_function = MXTensor.implements_torch_function


def _as_weight(b):
    """mm / addmm receive the transposed view [K, N] of an [N, K] weight (reference: linear passes args[1].t()); the kernels take [N, K]."""
    assert isinstance(b, MXTensor) and b.qdata.dim() == 2, "expected a 2-D MXTensor operand"
    return b if b.qdata.is_contiguous() else _transpose(b)


def _transpose(t):
    return t._with(t.qdata.t(), t.scale.t())


def _addmm_mx(a, w, bias):
    """reference _addmm_mx_dispatch (:760-841) with w the [N, K] weight: a plain activation is cast with the weight's act_quant_kwargs."""
    if not isinstance(a, MXTensor):
        assert w.act_quant_kwargs is not None, "weight-only quant not yet supported"
        k = w.act_quant_kwargs
        pref_a = k.kernel_preference
    else:
        k = None
        pref_a = a.kernel_preference
    assert pref_a == w.kernel_preference, "only same kernel preference is supported"
    if w.kernel_preference == KernelPreference.EMULATED:
        if k is not None:
            a = MXTensor.to_mx(a.contiguous(), k.elem_dtype, k.block_size, k.scaling_mode, k.kernel_preference)
        a_hp = a.dequantize(a.orig_dtype)
        b_hp = w.dequantize(w.orig_dtype).t()
        return aten.addmm.default(bias, a_hp, b_hp) if bias is not None else aten.mm.default(a_hp, b_hp)
    if w.kernel_preference not in (KernelPreference.AUTO, KernelPreference.TORCH):
        raise NotImplementedError(f"MXTensor on MI355X runs KernelPreference AUTO / TORCH (the HIP kernels) or EMULATED, got "
                                  f"{w.kernel_preference}")
    fmt = ops.mx_fmt(w.elem_dtype)
    from ..torch_ops import kernels

    if isinstance(a, MXTensor):
        assert a.elem_dtype == w.elem_dtype, "activation and weight element dtypes must match"
        y = kernels(a.qdata).mx_mm(a.qdata.contiguous(), a.scale, w.qdata, w.scale, bias, fmt)
        return y.to(a.orig_dtype)
    assert k.elem_dtype == w.elem_dtype, "For now - we only support matching input/weight dtypes."
    if k.block_size != BLOCK:
        raise NotImplementedError(f"MXTensor on MI355X implements block_size 32 only, got {k.block_size}")
    if a.dtype != torch.bfloat16:
        raise NotImplementedError(f"MXTensor linear on MI355X takes bfloat16 activations, got {a.dtype}: cast the activation explicitly "
                                  "(x.to(torch.bfloat16)) if that rounding is acceptable")
    if bias is not None and bias.dtype != torch.bfloat16:
        bias = bias.to(torch.bfloat16)
    mode = getattr(k.scaling_mode, "value", k.scaling_mode)
    return kernels(a).mx_linear(a.contiguous(), w.qdata, w.scale, bias, fmt, mode)


@implements(aten.linear.default)
@implements_torch_function(F.linear)
def _(func, types, args, kwargs):
    """reference :864-882"""
    a, w = args[0], args[1]
    bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
    assert isinstance(w, MXTensor)
    a2 = a.reshape(-1, a.shape[-1])
    res = _addmm_mx(a2, w, bias)
    return res.reshape(*a.shape[:-1], res.shape[-1])


@implements([aten.mm.default, aten.matmul.default])
@implements_torch_function([torch.mm, torch.matmul])
def _(func, types, args, kwargs):
    """reference :846-852"""
    return _addmm_mx(args[0], _as_weight(args[1]), None)


@implements(aten.addmm.default)
@implements_torch_function(torch.addmm)
def _(func, types, args, kwargs):
    """reference :855-861"""
    assert kwargs.get("alpha", 1) == 1 and kwargs.get("beta", 1) == 1, "only alpha = beta = 1 is supported"
    return _addmm_mx(args[1], _as_weight(args[2]), args[0])


@implements(aten.t.default)
def _(func, types, args, kwargs):
    """reference :885-899"""
    return _transpose(args[0])


@implements(aten.view.default)
def _(func, types, args, kwargs):
    """reference :922-939: the qdata is viewed (fp4: the last dimension halved), the scale kept"""
    t, size = args[0], list(args[1])
    if t.elem_dtype == torch.float4_e2m1fn_x2:
        if t.qdata.is_contiguous():
            size[-1] = size[-1] // 2 if size[-1] != -1 else -1
        else:
            size[0] = size[0] // 2 if size[0] != -1 else -1
    return t._with(t.qdata.view(size), t.scale)


torch.serialization.add_safe_globals([MXTensor, QuantizeTensorToMXKwargs])


@dataclass
class MXDynamicActivationMXWeightConfig(AOBaseConfig):
    """reference inference_workflow.py:80-119 (same fields, defaults and asserts).  e4m3 (MXFP8) and e2m1 (MXFP4) elements, block 32;
    AUTO runs the MI355X kernels, EMULATED the reference's dequantise-then-mm."""

    block_size: int = 32
    activation_dtype: object = torch.float8_e4m3fn
    weight_dtype: object = torch.float8_e4m3fn
    kernel_preference: KernelPreference = KernelPreference.AUTO
    scaling_mode: ScaleCalculationMode = ScaleCalculationMode.RCEIL

    def __post_init__(self):
        assert self.activation_dtype == self.weight_dtype, "For now - we only support matching input/weight dtypes."
        _validate_elem_dtype(self.activation_dtype)
        _validate_elem_dtype(self.weight_dtype)


@register_quantize_module_handler(MXDynamicActivationMXWeightConfig)
def _mx_inference_linear_transform(module: nn.Module, config: MXDynamicActivationMXWeightConfig, *, parameter_name: str = "weight"):
    """reference inference_workflow.py:126-171; the scales are kept row-major (is_swizzled_scales=False)."""
    weight = getattr(module, parameter_name)
    assert weight.dtype == torch.bfloat16, f"Only supporting bf16 out dtype for now, got {weight.dtype}"
    act_quant_kwargs = QuantizeTensorToMXKwargs(elem_dtype=config.activation_dtype, block_size=config.block_size,
                                                kernel_preference=config.kernel_preference, is_swizzled_scales=False,
                                                scaling_mode=config.scaling_mode)
    quantized_weight = MXTensor.to_mx(weight.detach().contiguous(), config.weight_dtype, block_size=config.block_size,
                                      kernel_preference=config.kernel_preference, act_quant_kwargs=act_quant_kwargs,
                                      is_swizzled_scales=False, scaling_mode=config.scaling_mode)
    setattr(module, parameter_name, nn.Parameter(quantized_weight, requires_grad=False))
    return module
