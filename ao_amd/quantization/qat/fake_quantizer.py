"""Fake quantizers (reference: torchao/quantization/qat/fake_quantizer.py:50-187): modules that replace a tensor by the values its
low-bit codes stand for, so that training sees the quantization error.  Each is one autograd Function over two HIP launches
(ao_amd/csrc/qat_kernels.hip): the forward saves only its input, the backward makes the range, the scale and the codes again.

Eager only, like the other training Functions here; bf16 tensors on the GPU (there is no CPU fallback).
"""
import torch

from ... import ops
from .fake_quantize_config import FakeQuantizeConfigBase, Float8FakeQuantizeConfig, Int4WeightFakeQuantizeConfig


class _Int4WeightFakeQuantize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, group_size):
        ctx.save_for_backward(w)
        ctx.group_size = group_size
        return ops.qat_int4_fake_quantize(w, group_size)

    @staticmethod
    def backward(ctx, grad_out):
        (w,) = ctx.saved_tensors
        return ops.qat_int4_fake_quantize_bwd(w, grad_out, ctx.group_size), None


class _Float8FakeQuantizeRowwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, hp_value_lb, hp_value_ub):
        ctx.save_for_backward(x)
        ctx.bounds = (hp_value_lb, hp_value_ub)
        return ops.qat_fp8_fake_quantize_rowwise(x, hp_value_lb, hp_value_ub)

    @staticmethod
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        return ops.qat_fp8_fake_quantize_rowwise_bwd(x, grad_out, *ctx.bounds), None, None


class FakeQuantizerBase(torch.nn.Module):
    """Generic module for applying fake quantization to a tensor, as specified in the config."""

    config: FakeQuantizeConfigBase

    def __repr__(self) -> str:
        return f"{type(self).__name__}({self.config})"

    @staticmethod
    def from_config(config: FakeQuantizeConfigBase) -> "FakeQuantizerBase":
        if isinstance(config, Int4WeightFakeQuantizeConfig):
            return Int4WeightFakeQuantizer(config)
        if isinstance(config, Float8FakeQuantizeConfig):
            return Float8FakeQuantizer(config)
        raise ValueError(f"Unknown config type: {config}")


class Float8FakeQuantizer(FakeQuantizerBase):
    """float8 e4m3 fake quantization, one scale per row of the last dimension (reference :73-98).  Its gradient is the chain's with every
    cast straight-through."""

    def __init__(self, config: Float8FakeQuantizeConfig):
        super().__init__()
        self.config = config
        self.enabled = True

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.enabled:
            return x
        return _Float8FakeQuantizeRowwise.apply(x, self.config.hp_value_lb, self.config.hp_value_ub)


class Int4WeightFakeQuantizer(FakeQuantizerBase):
    """int4 weight fake quantization with Int4Tensor's numerics under bf16 activations (reference :101-187, _bf16_activations_forward)."""

    def __init__(self, config: Int4WeightFakeQuantizeConfig):
        super().__init__()
        self.config = config
        self.enabled = True

    def forward(self, w: torch.Tensor) -> torch.Tensor:
        if not self.enabled:
            return w
        return _Int4WeightFakeQuantize.apply(w, self.config.group_size)
