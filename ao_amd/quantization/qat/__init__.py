"""Quantization-aware training (mirror of torchao.quantization.qat): fake quantizers on fused HIP kernels, FakeQuantizedLinear, QATConfig."""
from .api import QATConfig, QATStep
from .fake_quantize_config import (
    FakeQuantizeConfigBase,
    Float8FakeQuantizeConfig,
    Int4WeightFakeQuantizeConfig,
)
from .fake_quantizer import FakeQuantizerBase, Float8FakeQuantizer, Int4WeightFakeQuantizer
from .linear import FakeQuantizedLinear

__all__ = [
    "QATConfig",
    "QATStep",
    "FakeQuantizeConfigBase",
    "Float8FakeQuantizeConfig",
    "Int4WeightFakeQuantizeConfig",
    "FakeQuantizerBase",
    "Float8FakeQuantizer",
    "Int4WeightFakeQuantizer",
    "FakeQuantizedLinear",
]
