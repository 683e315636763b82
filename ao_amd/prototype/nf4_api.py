"""NF4WeightOnlyConfig and its quantize_ handler (reference torchao/prototype/_nf4tensor_api.py:15-39): every matching linear's weight
becomes nn.Parameter(NF4Tensor, requires_grad=False) -- the frozen base weight of QLoRA (ao_amd/quantization/nf4_tensor.py)."""
from dataclasses import dataclass

import torch.nn as nn

from ..quantization.config import AOBaseConfig
from ..quantization.nf4_tensor import NF4Tensor
from ..quantization.quant_api import register_quantize_module_handler

__all__ = ["NF4WeightOnlyConfig", "nf4_weight_only"]


@dataclass
class NF4WeightOnlyConfig(AOBaseConfig):
    """reference _nf4tensor_api.py:15-22 (same fields and defaults)"""

    block_size: int = 64
    scaler_block_size: int = 256


# for bc (reference :25-26)
nf4_weight_only = NF4WeightOnlyConfig


@register_quantize_module_handler(NF4WeightOnlyConfig)
def _nf4_weight_only_transform(module: nn.Module, config: NF4WeightOnlyConfig, *, parameter_name: str = "weight"):
    """reference :29-39"""
    new_weight = NF4Tensor.from_tensor(getattr(module, parameter_name), config.block_size, config.scaler_block_size)
    setattr(module, parameter_name, nn.Parameter(new_weight, requires_grad=False))
    return module
