"""BitNet b1.58 (https://arxiv.org/abs/2402.17764; mirrors torchao/prototype/quantized_training/bitnet.py) on the MI355X.

Training: `quantize_(model, BitNetTrainingConfig())` wraps each linear's bf16 weight in BitNetTrainingLinearWeight; F.linear on it casts
the activation to int8 per row, the weight to ternary values under its tensor-wise abs-mean, and multiplies them on the int8 MFMA with
the weight packed four to a byte (csrc/bitnet_kernels.hip).  The backward is the reference's high-precision one, on torch matmuls.
The Function saves the PACKED weight where the reference saves an int8 one: a quarter of the bytes, the same gradients.

Inference (this library's addition; the reference has no inference entry): `quantize_(model, BitNetInferenceConfig())` freezes a linear,
plain or under training, into a BitNetPacked2bitLinearWeight.

Left out, and refused by name: the FSDP2 / DTensor hooks (fsdp_pre_all_gather, fsdp_post_all_gather, precompute_bitnet_scale_for_fsdp),
the autocast branch, float16 and float32 weights or activations, and a K that is no multiple of 64."""
from typing import Optional

import torch
import torch.nn.functional as F
import torch.utils._pytree as pytree
from torch import Tensor, nn

from ao_amd import ops, torch_ops  # noqa: F401  (torch_ops registers ao_mi355::bitnet_linear)

from ...quantization.config import AOBaseConfig
from ...quantization.quant_api import register_quantize_module_handler

aten = torch.ops.aten

_NO_FSDP = "BitNet on the MI355X has no FSDP2 / DTensor support: {} is not built"


def get_bitnet_scale(x: Tensor) -> Tensor:
    """Tensor-wise abs-mean, always fp32: a 0-dim tensor on the device (ops.bitnet_absmean: float64 sum in a fixed order)."""
    return ops.bitnet_absmean(x)


def quantize_bitnet_weight(w: Tensor, scale: Tensor, eps: float = 1e-5) -> Tensor:
    """clip(round(w / max(scale, eps)), -1, 1) as int8.  The kernel's eps is the reference's default."""
    if eps != 1e-5:
        raise NotImplementedError(f"quantize_bitnet_weight: eps={eps} is not built, the kernel clips the scale at 1e-5")
    return ops.bitnet_quantize_weight(w, scale.to(torch.float32), with_int8=True)[1]


def _pack_i2_in_i8(x: Tensor) -> Tensor:
    """int8 [N, K] of 2-bit values -> int8 [N, K / 4]: the value at k = 4j + s goes to bits 7 - 2s .. 6 - 2s of byte j."""
    q = x.reshape(x.shape[0], -1, 4)
    return (q[..., 0] << 6) | ((q[..., 1] & 3) << 4) | ((q[..., 2] & 3) << 2) | (q[..., 3] & 3)


def _unpack_i2_in_i8(x: Tensor) -> Tensor:
    """int8 [N, K / 4] -> int8 [N, K]; the int8 shifts wrap and sign-extend, so each field reads as -2 .. 1."""
    return torch.stack([(x << s) >> 6 for s in (0, 2, 4, 6)], dim=-1).reshape(x.shape[0], -1)


def precompute_bitnet_scale_for_fsdp(module: nn.Module):
    raise NotImplementedError(_NO_FSDP.format("precompute_bitnet_scale_for_fsdp"))


def _check_bf16(what: str, t: Tensor):
    if t.dtype != torch.bfloat16:
        raise NotImplementedError(f"BitNet: {what} must be bfloat16, got {t.dtype} (float16 and float32 are not built)")


def _refuse_autocast():
    if torch.is_autocast_enabled("cuda"):
        raise NotImplementedError("BitNet: the autocast branch is not built; run the model in bfloat16 without autocast")


def _linear_args(args, kwargs):
    bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
    return args[0], args[1], bias


def _backward(ctx, grad_output):
    """The reference's high-precision backward: both gradients from the quantized operands, on torch matmuls."""
    input_i8, row_scale, packed, tensor_scale = ctx.saved_tensors
    grad_input = grad_weight = grad_bias = None
    batch_dims = grad_output.shape[:-1]
    grad_output = grad_output.reshape(-1, packed.shape[0])
    if ctx.needs_input_grad[0]:
        grad_input = ((grad_output @ ops.bitnet_dequantize(packed)) * tensor_scale).view(*batch_dims, packed.shape[1] * 4)
    if ctx.needs_input_grad[1]:
        grad_weight = grad_output.T @ (input_i8 * row_scale.view(-1, 1))
    if ctx.needs_input_grad[2]:
        grad_bias = grad_output.sum(0)
    return grad_input, grad_weight, grad_bias


class BitNetTrainingLinearWeight(Tensor):
    """A wrapper of the bf16 weight whose F.linear is the BitNet forward; every other op runs on the plain tensor."""

    @staticmethod
    @torch._dynamo.disable
    def __new__(cls, data: Tensor, precomputed_scale: Optional[Tensor] = None):
        return Tensor._make_wrapper_subclass(cls, data.shape, dtype=data.dtype, device=data.device)

    @torch._dynamo.disable
    def __init__(self, data: Tensor, precomputed_scale: Optional[Tensor] = None):
        self._data = data
        self._precomputed_scale = precomputed_scale  # (kept for the reference's signature: only its FSDP hooks read it)

    def __tensor_flatten__(self):
        return (["_data", "_precomputed_scale"] if self._precomputed_scale is not None else ["_data"]), []

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size=None, outer_stride=None):
        return cls(tensor_data_dict["_data"], tensor_data_dict.get("_precomputed_scale", None), *tensor_attributes)

    def __repr__(self):
        return f"{self.__class__.__name__}(data={self._data})"

    _PRESERVED = None  # the ops whose result stays wrapped (filled below)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is F.linear:
            _refuse_autocast()
            return _BitNetTrainingLinear.apply(*_linear_args(args, kwargs))
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)

    @classmethod
    def __torch_dispatch__(cls, func, types, args, kwargs=None):
        out = func(*pytree.tree_map_only(cls, lambda x: x._data, args), **pytree.tree_map_only(cls, lambda x: x._data, kwargs or {}))
        if func is aten.copy_.default:
            return args[0]  # the original object
        if func in cls._PRESERVED:
            return pytree.tree_map_only(Tensor, lambda x: cls(x), out)  # (the precomputed scale does not travel through ops)
        return out

    def fsdp_pre_all_gather(self, mesh):
        raise NotImplementedError(_NO_FSDP.format("fsdp_pre_all_gather"))

    def fsdp_post_all_gather(self, all_gather_outputs, metadata, param_dtype, *, out=None):
        raise NotImplementedError(_NO_FSDP.format("fsdp_post_all_gather"))


BitNetTrainingLinearWeight._PRESERVED = {
    aten.t.default, aten.detach.default, aten.empty_like.default, aten.new_zeros.default, aten.slice.Tensor, aten.view.default,
    aten.as_strided.default, aten._to_copy.default, aten._pin_memory.default, aten.split.Tensor, aten.clone.default,
}


class _BitNetTrainingLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input: Tensor, weight: BitNetTrainingLinearWeight, bias: Optional[Tensor] = None):
        w = weight._data
        _check_bf16("the weight", w)
        _check_bf16("the activation", input)
        input_i8, row_scale = ops.bitnet_quantize_act(input.reshape(-1, w.shape[1]))
        scale, tensor_scale = ops.bitnet_absmean(w, with_bf16=True)  # fp32 for the weight cast, bf16 for the matmul and the backward
        packed = ops.bitnet_quantize_weight(w, scale)
        ctx.save_for_backward(input_i8, row_scale, packed, tensor_scale)
        return ops.bitnet_mm(input_i8, packed, row_scale, tensor_scale, bias).view(*input.shape[:-1], w.shape[0])

    backward = staticmethod(_backward)


class BitNetTrainingConfig(AOBaseConfig):
    pass


bitnet_training = BitNetTrainingConfig  # for bc


@register_quantize_module_handler(BitNetTrainingConfig)
def _bitnet_training_transform(module: nn.Module, config: BitNetTrainingConfig) -> nn.Module:
    _check_bf16("the weight", module.weight)
    module.weight = nn.Parameter(BitNetTrainingLinearWeight(module.weight.detach()), requires_grad=True)
    return module


class BitNetPacked2bitLinearWeight(Tensor):
    """Ternary weights packed four to a byte (int_data int8 [N, K / 4], the bytes of _pack_i2_in_i8) and their 0-dim tensor scale."""

    @staticmethod
    @torch._dynamo.disable
    def __new__(cls, int_data: Tensor, scale: Tensor):
        n, kb = int_data.shape
        return Tensor._make_wrapper_subclass(cls, (n, kb * 4), dtype=scale.dtype, device=scale.device)

    @torch._dynamo.disable
    def __init__(self, int_data: Tensor, scale: Tensor):
        assert int_data.dtype is torch.int8
        assert scale.shape == ()
        self.int_data = int_data
        self.scale = scale

    @classmethod
    def from_hp(cls, w: Tensor) -> "BitNetPacked2bitLinearWeight":
        """The frozen form of a bf16 weight [N, K]: the bytes and the scale the training forward would use."""
        _check_bf16("the weight", w)
        scale, tensor_scale = ops.bitnet_absmean(w.detach(), with_bf16=True)
        return cls(ops.bitnet_quantize_weight(w.detach(), scale), tensor_scale)

    def __tensor_flatten__(self):
        return ["int_data", "scale"], []

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size=None, outer_stride=None):
        return cls(tensor_data_dict["int_data"], tensor_data_dict["scale"], *tensor_attributes)

    def __repr__(self):
        return f"{self.__class__.__name__}(data={self.dequantize()})"

    def dequantize(self, out_dtype=None):
        out = ops.bitnet_dequantize(self.int_data).to(self.scale.dtype) * self.scale
        return out if out_dtype is None else out.to(out_dtype)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is F.linear:
            return _BitNetPacked2bitLinear.apply(*_linear_args(args, kwargs))
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)

    @classmethod
    def __torch_dispatch__(cls, func, types, args, kwargs=None):
        if func in (aten.detach.default, aten.clone.default):
            return cls(func(args[0].int_data, *args[1:], **(kwargs or {})), func(args[0].scale, *args[1:], **(kwargs or {})))
        raise NotImplementedError(f"{cls.__name__} dispatch: attempting to run {func}, this is not supported")


class _BitNetPacked2bitLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input: Tensor, weight: BitNetPacked2bitLinearWeight, bias: Optional[Tensor] = None):
        _check_bf16("the activation", input)
        _check_bf16("the weight's scale", weight.scale)
        packed, tensor_scale = weight.int_data, weight.scale
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            input_i8, row_scale = ops.bitnet_quantize_act(input.reshape(-1, weight.shape[1]))
            ctx.save_for_backward(input_i8, row_scale, packed, tensor_scale)
            return ops.bitnet_mm(input_i8, packed, row_scale, tensor_scale, bias).view(*input.shape[:-1], weight.shape[0])
        return torch_ops.kernels(input).bitnet_linear(input, packed, tensor_scale, bias)

    backward = staticmethod(_backward)


class BitNetInferenceConfig(AOBaseConfig):
    """Freeze a linear into its packed 2-bit form: a bf16 weight, plain or a BitNetTrainingLinearWeight."""


@register_quantize_module_handler(BitNetInferenceConfig)
def _bitnet_inference_transform(module: nn.Module, config: BitNetInferenceConfig) -> nn.Module:
    w = module.weight
    w = w._data if isinstance(w, BitNetTrainingLinearWeight) else w
    if w.shape[1] % 64 != 0:
        raise ValueError(f"BitNetInferenceConfig: {ops.bitnet_mm_fits(1, w.shape[0], w.shape[1])}")
    module.weight = nn.Parameter(BitNetPacked2bitLinearWeight.from_hp(w.detach()), requires_grad=False)
    return module
