"""OptimStateFp8: an Adam moment as e4m3fn codes with one fp32 scale per block of the flat tensor.  The fields of
torchao/optim/subclass_fp8.py (codes, scale); the casts are the kernels of csrc/optim_kernels.hip."""
import torch
from torch import Tensor
from torch.serialization import add_safe_globals

from ..quantization.base_tensor import LowBitTensorBase
from . import _state_ops
from .quant_utils import FP8

DTYPE = torch.float8_e4m3fn


class OptimStateFp8(LowBitTensorBase):
    tensor_attrs = ["codes", "scale"]
    tensor_data_names = tensor_attrs

    # dtype is the appearance dtype only
    @staticmethod
    def __new__(cls, codes: Tensor, scale: Tensor, dtype=None):
        return Tensor._make_wrapper_subclass(cls, codes.shape, device=codes.device, dtype=dtype)

    def __init__(self, codes: Tensor, scale: Tensor, dtype=None):
        """codes: float8_e4m3fn in the shape of the float tensor; scale: fp32 [numel / block_size] over the FLAT tensor."""
        assert codes.dtype is DTYPE
        assert scale.ndim == 1
        self.codes, self.scale = codes, scale
        self.block_size = codes.numel() // scale.numel()

    def __tensor_flatten__(self):
        return self.tensor_attrs, [self.dtype]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size=None, outer_stride=None):
        return cls(*[tensor_data_dict[name] for name in cls.tensor_attrs], *tensor_attributes)

    @classmethod
    def zeros(cls, shape, block_size: int = 256, device=None, dtype=None):
        codes = torch.zeros(shape, dtype=DTYPE, device=device)
        scale = torch.zeros(codes.numel() // block_size, device=device)
        return cls(codes, scale, dtype=dtype)

    def dequantize(self, output_dtype=None):
        return _state_ops.dequantize_state(self, output_dtype)

    # ---- what _state_ops asks of a state class ----
    def _format(self):
        return FP8

    def _qmap(self):
        return None

    def _fields(self):
        return self.codes, self.scale

    def _layout(self):
        return (self.block_size, tuple(self.shape))

    def _rewrap(self, codes, scale, dtype=None):
        return OptimStateFp8(codes, scale, dtype=dtype)

    def _view(self, shape):
        return OptimStateFp8(self.codes.view(shape), self.scale, dtype=self.dtype)

    def _slice(self, start, end, stride):
        b = self.block_size
        return OptimStateFp8(self.codes[start:end], self.scale[start * stride // b:end * stride // b], dtype=self.dtype)

    def __repr__(self):
        return (f"{self.__class__.__name__}(block_size={self.block_size}, shape={tuple(self.shape)}, dtype={self.dtype}, device={self.device}, "
                f"requires_grad={self.requires_grad})")


_state_ops.register_state_ops(OptimStateFp8)
add_safe_globals([OptimStateFp8])
