"""OptimState4bit: an Adam moment as 4-bit codes into a 16-entry table, two a byte (element 2i in the HIGH nibble), one fp32 scale per
block of the flat tensor (arXiv 2309.01507).  The fields of torchao/optim/subclass_4bit.py (flat codes, scale, qmap, signed, _shape); the
casts are the kernels of csrc/optim_kernels.hip."""
import math

import torch
from torch import Tensor
from torch.serialization import add_safe_globals

from ..quantization.base_tensor import LowBitTensorBase
from . import _state_ops
from .quant_utils import make_qmap, table_format


class OptimState4bit(LowBitTensorBase):
    tensor_attrs = ["codes", "scale", "qmap"]
    tensor_data_names = tensor_attrs

    # dtype is the appearance dtype only
    @staticmethod
    def __new__(cls, codes: Tensor, scale: Tensor, qmap: Tensor, signed: bool, shape, dtype=None):
        return Tensor._make_wrapper_subclass(cls, shape, device=codes.device, dtype=dtype)

    def __init__(self, codes: Tensor, scale: Tensor, qmap: Tensor, signed: bool, shape, dtype=None):
        """codes: packed uint8, FLAT [numel / 2]; scale: fp32 [numel / block_size]; qmap: the 16 fp32 table values; shape: the float tensor's."""
        assert codes.dtype is torch.uint8
        assert codes.ndim == 1
        assert scale.ndim == 1
        assert qmap.dtype is torch.float32
        self.codes, self.scale, self.qmap, self.signed = codes, scale, qmap, signed
        self._shape = shape
        self.block_size = codes.numel() * 2 // scale.numel()

    def __tensor_flatten__(self):
        return self.tensor_attrs, [self.signed, self._shape, self.dtype]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size=None, outer_stride=None):
        return cls(*[tensor_data_dict[name] for name in cls.tensor_attrs], *tensor_attributes)

    @classmethod
    def zeros(cls, shape, signed: bool = True, block_size: int = 128, device=None, dtype=None):
        shape = (shape,) if isinstance(shape, int) else shape
        n = math.prod(shape)
        codes = torch.zeros(n // 2, dtype=torch.uint8, device=device)
        scale = torch.zeros(n // block_size, device=device)
        return cls(codes, scale, make_qmap(4, signed, device), signed, shape, dtype=dtype)

    def dequantize(self, output_dtype=None):
        return _state_ops.dequantize_state(self, output_dtype)

    # ---- what _state_ops asks of a state class ----
    def _format(self):
        return table_format(4, self.signed)

    def _qmap(self):
        return self.qmap

    def _fields(self):
        return self.codes, self.scale, self.qmap

    def _layout(self):
        return (self.signed, self.block_size, tuple(self._shape))

    def _rewrap(self, codes, scale, qmap, dtype=None):
        return OptimState4bit(codes, scale, qmap, self.signed, self._shape, dtype=dtype)

    def _view(self, shape):
        shape = tuple(shape)
        if shape.count(-1) == 1:
            known = -math.prod(shape)
            shape = tuple(math.prod(self._shape) // known if s == -1 else s for s in shape)
        if math.prod(shape) != math.prod(self._shape):
            raise ValueError(f"{self.__class__.__name__} only supports view() to a shape of the same element count, got {shape}")
        return OptimState4bit(self.codes, self.scale, self.qmap, self.signed, shape, dtype=self.dtype)

    def _slice(self, start, end, stride):
        b = self.block_size
        return OptimState4bit(self.codes[start * stride // 2:end * stride // 2], self.scale[start * stride // b:end * stride // b], self.qmap.clone(),
                              self.signed, (end - start,) + tuple(self.shape[1:]), dtype=self.dtype)

    def __repr__(self):
        return (f"{self.__class__.__name__}(signed={self.signed}, block_size={self.block_size}, shape={tuple(self.shape)}, dtype={self.dtype}, "
                f"device={self.device}, requires_grad={self.requires_grad})")


_state_ops.register_state_ops(OptimState4bit)
add_safe_globals([OptimState4bit])
