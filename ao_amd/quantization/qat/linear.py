"""FakeQuantizedLinear (reference: torchao/quantization/qat/linear.py:42-155): an nn.Linear whose activation and weight pass through fake
quantizers before PyTorch's own bf16 matmul."""
from typing import Optional

import torch
import torch.nn.functional as F

from .fake_quantize_config import FakeQuantizeConfigBase
from .fake_quantizer import FakeQuantizerBase


class FakeQuantizedLinear(torch.nn.Linear):
    """General linear layer with fake quantized weights and activations; either config may be None (that operand stays as it is)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, activation_config: Optional[FakeQuantizeConfigBase] = None,
                 weight_config: Optional[FakeQuantizeConfigBase] = None, *args, **kwargs) -> None:
        super().__init__(in_features, out_features, bias, *args, **kwargs)
        self.activation_fake_quantizer = None if activation_config is None else FakeQuantizerBase.from_config(activation_config)
        self.weight_fake_quantizer = None if weight_config is None else FakeQuantizerBase.from_config(weight_config)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.activation_fake_quantizer is not None:
            x = self.activation_fake_quantizer(x)
        w = self.weight if self.weight_fake_quantizer is None else self.weight_fake_quantizer(self.weight)
        return F.linear(x, w, self.bias)

    def to_linear(self) -> torch.nn.Linear:
        """A plain nn.Linear over the SAME parameters."""
        new_linear = torch.nn.Linear(self.in_features, self.out_features, self.bias is not None, device=self.weight.device,
                                     dtype=self.weight.dtype)
        if self.weight.device != torch.device("meta"):  # (a model on the meta device has nothing to share)
            new_linear.weight = self.weight
            new_linear.bias = self.bias
        return new_linear

    @classmethod
    def from_linear(cls, mod: torch.nn.Linear, activation_config: Optional[FakeQuantizeConfigBase] = None,
                    weight_config: Optional[FakeQuantizeConfigBase] = None):
        """A FakeQuantizedLinear over the SAME parameters as `mod`."""
        new_linear = FakeQuantizedLinear(mod.in_features, mod.out_features, mod.bias is not None, activation_config=activation_config,
                                         weight_config=weight_config, device=mod.weight.device, dtype=mod.weight.dtype)
        if mod.weight.device != torch.device("meta"):
            new_linear.weight = mod.weight
            new_linear.bias = mod.bias
        return new_linear
