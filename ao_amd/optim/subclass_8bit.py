"""OptimState8bit: an Adam moment as 8-bit codes into a 256-entry table with one fp32 scale per block of the flat tensor
(arXiv 2110.02861).  The fields of torchao/optim/subclass_8bit.py (codes, scale, qmap, signed), so the tensors of a state dict carry over;
the casts are the kernels of csrc/optim_kernels.hip."""
import torch
from torch import Tensor
from torch.serialization import add_safe_globals

from ..quantization.base_tensor import LowBitTensorBase
from . import _state_ops
from .quant_utils import make_qmap, table_format


class OptimState8bit(LowBitTensorBase):
    tensor_attrs = ["codes", "scale", "qmap"]
    tensor_data_names = tensor_attrs

    # dtype is the appearance dtype only: what the rest of PyTorch sees
    @staticmethod
    def __new__(cls, codes: Tensor, scale: Tensor, qmap: Tensor, signed: bool, dtype=None):
        return Tensor._make_wrapper_subclass(cls, codes.shape, device=codes.device, dtype=dtype)

    def __init__(self, codes: Tensor, scale: Tensor, qmap: Tensor, signed: bool, dtype=None):
        """codes: uint8 in the shape of the float tensor; scale: fp32 [numel / block_size] over the FLAT tensor (the last dimension need not be a
        multiple of the block size); qmap: the 256 fp32 table values; signed: which of the two tables."""
        assert codes.dtype is torch.uint8
        assert scale.ndim == 1
        assert qmap.dtype is torch.float32
        self.codes, self.scale, self.qmap, self.signed = codes, scale, qmap, signed
        self.block_size = codes.numel() // scale.numel()

    def __tensor_flatten__(self):
        return self.tensor_attrs, [self.signed, self.dtype]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size=None, outer_stride=None):
        return cls(*[tensor_data_dict[name] for name in cls.tensor_attrs], *tensor_attributes)

    @classmethod
    def zeros(cls, shape, signed: bool = True, block_size: int = 256, device=None, dtype=None):
        codes = torch.zeros(shape, dtype=torch.uint8, device=device)
        scale = torch.zeros(codes.numel() // block_size, device=device)
        return cls(codes, scale, make_qmap(8, signed, device), signed, dtype=dtype)

    def dequantize(self, output_dtype=None):
        return _state_ops.dequantize_state(self, output_dtype)

    # ---- what _state_ops asks of a state class ----
    def _format(self):
        return table_format(8, self.signed)

    def _qmap(self):
        return self.qmap

    def _fields(self):
        return self.codes, self.scale, self.qmap

    def _layout(self):
        return (self.signed, self.block_size, tuple(self.shape))

    def _rewrap(self, codes, scale, qmap, dtype=None):
        return OptimState8bit(codes, scale, qmap, self.signed, dtype=dtype)

    def _view(self, shape):
        return OptimState8bit(self.codes.view(shape), self.scale, self.qmap, self.signed, dtype=self.dtype)

    def _slice(self, start, end, stride):
        b = self.block_size
        return OptimState8bit(self.codes[start:end], self.scale[start * stride // b:end * stride // b], self.qmap.clone(), self.signed, dtype=self.dtype)

    def __repr__(self):
        return (f"{self.__class__.__name__}(signed={self.signed}, block_size={self.block_size}, shape={tuple(self.shape)}, dtype={self.dtype}, "
                f"device={self.device}, requires_grad={self.requires_grad})")


_state_ops.register_state_ops(OptimState8bit)
add_safe_globals([OptimState8bit])
