"""Intx weights, int1 .. int8 (reference: torchao/quantization/quantize_/workflows/intx/intx_unpacked_to_int8_tensor.py).

IntxUnpackedToInt8Tensor is the reference's tensor: codes as int8 [N, K] inside the range of target_dtype, scale and int8 zero_point
[N, K / g].  from_hp is ONE launch (ops.intx_quantize, the reference's bf16 arithmetic byte for byte) and F.linear is one launch that reads
the int8 codes in place and decodes them in registers (ops.intx_linear), where the reference dequantizes the whole weight on every call.
IntxBitPackedTensor is the device-packed sibling the reference lacks: the same scale / zero_point over b-bit codes in the layout
csrc/intx_kernels.hip states (b / 8 of a byte a weight), built with from_intx_unpacked_to_int8_tensor and converted back exactly.

Left out, and refused by name: HQQ_SCALE_ONLY, the CPU opaque packing formats, fp16 / fp32 weights, activations and scales, float
zero-points, 4-D conv weights, F.embedding, a K that is no multiple of 32 and a group size that is no multiple of 32 dividing K."""
import enum
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from ao_amd import ops, torch_ops  # noqa: F401  (torch_ops registers ao_mi355::intx_linear)

from .base_tensor import LowBitTensorBase
from .config import IntxChooseQParamsAlgorithm, IntxPackingFormat
from .quant_primitives import MappingType

aten = torch.ops.aten

_INT_DTYPES = [getattr(torch, f"int{b}") for b in range(1, 9)]


class IntxUnpackedToInt8TensorActivationQuantization(str, enum.Enum):
    INT8_ASYM_PER_TOKEN = "int8_asym_per_token"


def _bits(target_dtype) -> int:
    assert target_dtype in _INT_DTYPES, f"target_dtype must be torch.intx, where 1 <= x <= 8, but got {target_dtype}"
    return _INT_DTYPES.index(target_dtype) + 1


def _check_bf16(what: str, dtype):
    if dtype != torch.bfloat16:
        raise NotImplementedError(f"Intx on MI355X: {what} must be bfloat16, got {dtype} (float16 and float32 are not built)")


def _check_blocking(shape, block_size) -> int:
    """The group size of a 2-D weight's block_size (1, g): a multiple of 32 that divides K, itself a multiple of 32."""
    if len(shape) != 2:
        raise NotImplementedError(f"Intx on MI355X takes 2-D linear weights, got a {len(shape)}-D tensor (4-D conv weights are not built)")
    assert len(block_size) == 2, f"block_size {tuple(block_size)} must have the weight's two dimensions"
    n, k = shape
    g = int(block_size[1])
    if int(block_size[0]) != 1:
        raise NotImplementedError(f"Intx on MI355X: block_size must be (1, group_size), got {tuple(block_size)}")
    if k % 32 != 0:
        raise ValueError(f"Intx on MI355X: K={k} must be a multiple of 32 (a packed run is 32 weights)")
    if g < 32 or g % 32 != 0 or k % g != 0:
        raise ValueError(f"Intx on MI355X: the group size {g} must be a multiple of 32 that divides K={k}")
    return g


def _linear_args(args, kwargs):
    bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
    return args[0], args[1], bias


def _linear(x, w, codes, bias):
    """F.linear on either tensor: the activation fake quantization where the weight asks for it, then the fused linear."""
    if not x.is_cuda:
        raise RuntimeError(f"{type(w).__name__}: F.linear runs on the MI355X only; there is no CPU fallback")
    _check_bf16("the activation", x.dtype)
    _check_bf16("the weight's scale", w.scale.dtype)
    if w.zero_point.dtype != torch.int8:
        raise NotImplementedError(f"Intx on MI355X: zero_point must be int8, got {w.zero_point.dtype} (float zero-points are not built)")
    return torch_ops.kernels(x).intx_linear(x, codes, w.scale, w.zero_point, _bits(w.target_dtype), bias,
                                            w.activation_quantization is not None)


class IntxUnpackedToInt8Tensor(LowBitTensorBase):
    """qdata int8 [N, K], scale [N, K / g], zero_point int8 [N, K / g]; attributes target_dtype, block_size, dtype, activation_quantization."""

    tensor_data_names = ["qdata", "scale", "zero_point"]
    tensor_attribute_names = ["target_dtype", "block_size", "dtype", "activation_quantization"]

    def __new__(cls, qdata, scale, zero_point, target_dtype, block_size, dtype, activation_quantization):
        return torch.Tensor._make_wrapper_subclass(cls, qdata.shape, device=qdata.device, dtype=dtype, requires_grad=False)

    def __init__(self, qdata, scale, zero_point, target_dtype, block_size, dtype, activation_quantization):
        assert qdata.dtype == torch.int8, f"qdata dtype must be int8, but got {qdata.dtype}"
        _bits(target_dtype)
        assert len(block_size) == qdata.ndim
        n_blocks = tuple(qdata.shape[i] // block_size[i] for i in range(qdata.ndim))
        assert all(qdata.shape[i] % block_size[i] == 0 for i in range(qdata.ndim))
        assert tuple(scale.shape) == n_blocks, f"Expected scale to have shape {n_blocks} (inferred from block_size={block_size}), but got {scale.shape}"
        assert tuple(zero_point.shape) == n_blocks, (
            f"Expected zero_point to have shape {n_blocks} (inferred from block_size={block_size}), but got {zero_point.shape}")
        self.qdata, self.scale, self.zero_point = qdata, scale, zero_point
        self.target_dtype = target_dtype
        self.block_size = tuple(block_size)
        self.activation_quantization = activation_quantization

    def _quantization_type(self):
        return (f"target_dtype={self.target_dtype}, block_size={self.block_size}, shape={self.shape}, dtype={self.dtype}, "
                f"device={self.device}, activation_quantization={self.activation_quantization}")

    def to(self, *args, **kwargs):
        device, dtype, _, _ = torch._C._nn._parse_to(*args, **kwargs)
        dtype = self.dtype if dtype is None else dtype
        _check_bf16("the dtype of to()", dtype)
        device = self.device if device is None else device
        return IntxUnpackedToInt8Tensor(self.qdata.to(device), self.scale.to(device), self.zero_point.to(device), self.target_dtype,
                                        self.block_size, dtype, self.activation_quantization)

    @classmethod
    def from_hp(cls, hp_tensor: torch.Tensor, block_size: Tuple[int], target_dtype: torch.dtype, *,
                mapping_type: MappingType = MappingType.SYMMETRIC, activation_quantization=None,
                intx_choose_qparams_algorithm: Optional[IntxChooseQParamsAlgorithm] = IntxChooseQParamsAlgorithm.AFFINE,
                custom_scale: Optional[torch.Tensor] = None, custom_zero_point: Optional[torch.Tensor] = None):
        """reference :173-259.  AFFINE, or (algorithm None) quantize_affine under a custom scale and zero-point."""
        bits = _bits(target_dtype)
        if intx_choose_qparams_algorithm is not None:
            assert custom_scale is None, "custom_scale is not supported with intx_choose_qparams_algorithm"
            assert custom_zero_point is None, "custom_zero_point is not supported with intx_choose_qparams_algorithm"
            if IntxChooseQParamsAlgorithm(intx_choose_qparams_algorithm) == IntxChooseQParamsAlgorithm.HQQ_SCALE_ONLY:
                raise NotImplementedError("Intx on MI355X: IntxChooseQParamsAlgorithm.HQQ_SCALE_ONLY is not built; use AFFINE")
        else:
            assert custom_scale is not None, "custom_scale must be given"
            assert custom_zero_point is not None, "custom_zero_point must be given"
        _check_bf16("the weight", hp_tensor.dtype)
        g = _check_blocking(hp_tensor.shape, block_size)
        if activation_quantization is not None:
            activation_quantization = IntxUnpackedToInt8TensorActivationQuantization(activation_quantization)
        if custom_scale is not None:
            _check_bf16("custom_scale", custom_scale.dtype)
            if custom_zero_point.dtype != torch.int8:
                raise NotImplementedError(f"Intx on MI355X: custom_zero_point must be int8, got {custom_zero_point.dtype} (float zero-points are not built)")
            shape = (hp_tensor.shape[0], hp_tensor.shape[1] // g)
            custom_scale, custom_zero_point = custom_scale.reshape(shape), custom_zero_point.reshape(shape)
        qdata, scale, zero_point = ops.intx_quantize(hp_tensor.detach(), g, bits, MappingType(mapping_type).name, custom_scale, custom_zero_point)
        return cls(qdata, scale, zero_point, target_dtype, tuple(block_size), hp_tensor.dtype, activation_quantization)

    def dequantize(self):
        """dequantize_affine byte for byte: bf16((qdata - zero_point) * scale), one launch."""
        _check_blocking(self.shape, self.block_size)
        return ops.intx_dequantize(self.qdata, self.scale, self.zero_point, _bits(self.target_dtype))


@IntxUnpackedToInt8Tensor.implements(aten.linear.default)
@IntxUnpackedToInt8Tensor.implements_torch_function(F.linear)
def _(func, types, args, kwargs):
    x, w, bias = _linear_args(args, kwargs)
    return _linear(x, w, w.qdata, bias)


@IntxUnpackedToInt8Tensor.implements(aten.slice.Tensor)
def _(func, types, args, kwargs):
    """reference :383-435: start and end must sit on block boundaries of the sliced dimension."""
    self, dim, start, end, step = (list(args) + [0, None, None, 1][len(args) - 1:])[:5]
    assert step == 1
    start = 0 if start is None else start
    end = self.shape[dim] if end is None or end > self.shape[dim] else end
    bs = self.block_size[dim]
    assert start % bs == 0, f"slice args are incompatible with blocking: start={start} must be divisible by block_size[dim]={bs}"
    assert end % bs == 0, f"slice args are incompatible with blocking: end={end} must be divisible by block_size[dim]={bs}"
    qdata = aten.slice.Tensor(self.qdata, dim, start, end, step)
    scale = aten.slice.Tensor(self.scale, dim, start // bs, end // bs, step)
    zero_point = aten.slice.Tensor(self.zero_point, dim, start // bs, end // bs, step)
    block = tuple(qdata.shape[i] // scale.shape[i] for i in range(qdata.ndim))
    return IntxUnpackedToInt8Tensor(qdata, scale, zero_point, self.target_dtype, block, self.dtype, self.activation_quantization)


def _refuse(cls, what):
    def impl(func, types, args, kwargs):
        raise NotImplementedError(f"{cls.__name__} on MI355X: {what} is not built (linear weights only)")
    return impl


class IntxBitPackedTensor(LowBitTensorBase):
    """packed int32 [N, K / 32 * b] (b dwords a run of 32 weights: csrc/intx_kernels.hip), scale and zero_point as the unpacked tensor's."""

    tensor_data_names = ["packed", "scale", "zero_point"]
    tensor_attribute_names = ["target_dtype", "block_size", "dtype", "activation_quantization"]

    def __new__(cls, packed, scale, zero_point, target_dtype, block_size, dtype, activation_quantization):
        shape = (packed.shape[0], packed.shape[1] // _bits(target_dtype) * 32)
        return torch.Tensor._make_wrapper_subclass(cls, shape, device=packed.device, dtype=dtype, requires_grad=False)

    def __init__(self, packed, scale, zero_point, target_dtype, block_size, dtype, activation_quantization):
        assert packed.dtype == torch.int32 and packed.dim() == 2 and packed.shape[1] % _bits(target_dtype) == 0
        self.packed, self.scale, self.zero_point = packed, scale, zero_point
        self.target_dtype = target_dtype
        self.block_size = tuple(block_size)
        self.activation_quantization = activation_quantization

    def _quantization_type(self):
        return (f"target_dtype={self.target_dtype}, block_size={self.block_size}, shape={tuple(self.shape)}, dtype={self.dtype}, "
                f"device={self.device}, activation_quantization={self.activation_quantization}")

    @classmethod
    def from_intx_unpacked_to_int8_tensor(cls, t: IntxUnpackedToInt8Tensor) -> "IntxBitPackedTensor":
        _check_blocking(t.shape, t.block_size)
        if t.zero_point.dtype != torch.int8:
            raise NotImplementedError(f"Intx on MI355X: zero_point must be int8, got {t.zero_point.dtype} (float zero-points are not built)")
        return cls(ops.intx_pack(t.qdata, _bits(t.target_dtype)), t.scale, t.zero_point, t.target_dtype, t.block_size, t.dtype,
                   t.activation_quantization)

    def to_intx_unpacked_to_int8_tensor(self) -> IntxUnpackedToInt8Tensor:
        return IntxUnpackedToInt8Tensor(ops.intx_unpack(self.packed, _bits(self.target_dtype)), self.scale, self.zero_point, self.target_dtype,
                                        self.block_size, self.dtype, self.activation_quantization)

    def dequantize(self):
        return ops.intx_dequantize(self.packed, self.scale, self.zero_point, _bits(self.target_dtype))


@IntxBitPackedTensor.implements(aten.linear.default)
@IntxBitPackedTensor.implements_torch_function(F.linear)
def _(func, types, args, kwargs):
    x, w, bias = _linear_args(args, kwargs)
    return _linear(x, w, w.packed, bias)


for _cls in (IntxUnpackedToInt8Tensor, IntxBitPackedTensor):
    _cls.implements([aten.embedding.default])(_refuse(_cls, "F.embedding"))
    _cls.implements_torch_function(F.embedding)(_refuse(_cls, "F.embedding"))
    _cls.implements([aten.conv2d.default])(_refuse(_cls, "F.conv2d"))
    _cls.implements_torch_function(F.conv2d)(_refuse(_cls, "F.conv2d"))

torch.serialization.add_safe_globals([IntxUnpackedToInt8Tensor, IntxBitPackedTensor, IntxUnpackedToInt8TensorActivationQuantization,
                                      IntxPackingFormat, IntxChooseQParamsAlgorithm])
