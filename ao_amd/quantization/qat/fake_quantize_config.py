"""Fake-quantization configs (reference: torchao/quantization/qat/fake_quantize_config.py:40-102, 345-489).

Same names, same argument names and the reference's validation messages; what the reference accepts and MI355X does not run is refused
by name with NotImplementedError that says what works.
"""
import abc
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ..config import (
    AOBaseConfig,
    Float8DynamicActivationFloat8WeightConfig,
    Int4PackingFormat,
    Int4WeightOnlyConfig,
)
from ..granularity import Granularity, PerBlock, PerRow, PerTensor

e4m3_dtype = torch.float8_e4m3fn
_FLOAT8_TYPES = (torch.float8_e4m3fn, torch.float8_e5m2, torch.float8_e4m3fnuz, torch.float8_e5m2fnuz)


class FakeQuantizeConfigBase(abc.ABC):
    """Base class of the fake quantization configs."""


@dataclass
class Float8FakeQuantizeConfig(FakeQuantizeConfigBase):
    """float8 fake quantization targeting Float8Tensor (reference :48-78).  On MI355X: float8_e4m3fn, one scale per row of the last
    dimension.  hp_value_lb / hp_value_ub bound the row maximum the scale is calculated from."""

    dtype: torch.dtype = e4m3_dtype
    granularity: Granularity = PerRow()
    hp_value_lb: Optional[float] = None
    hp_value_ub: Optional[float] = None

    def __post_init__(self):
        if self.dtype not in _FLOAT8_TYPES:
            raise ValueError(f"{self.dtype} is not a float8 dtype")
        if isinstance(self.granularity, type):
            raise ValueError("Please specify the granularity object instead of the class, e.g. PerRow() instead of PerRow")
        if isinstance(self.granularity, PerBlock):
            raise NotImplementedError(
                f"Float8FakeQuantizeConfig(granularity={self.granularity}): blockwise float8 fake quantization is not implemented on "
                "MI355X; use PerRow(), the fake quantizer of Float8DynamicActivationFloat8WeightConfig(granularity=PerRow())")
        if type(self.granularity) not in [PerRow, PerTensor]:
            raise ValueError(f"Expected PerRow or PerTensor granularity, got {self.granularity}")
        if isinstance(self.granularity, PerTensor) or self.granularity.dim != -1:
            raise NotImplementedError(
                f"Float8FakeQuantizeConfig(granularity={self.granularity}): only PerRow() (one scale per row of the last dimension) is "
                "implemented on MI355X")
        if self.dtype != e4m3_dtype:
            raise NotImplementedError(
                f"Float8FakeQuantizeConfig(dtype={self.dtype}): only torch.float8_e4m3fn is implemented on MI355X (gfx950 casts OCP "
                "e4m3fn; the float8 linears it prepares for are e4m3fn)")


@dataclass
class Int4WeightFakeQuantizeConfig(FakeQuantizeConfigBase):
    """int4 weight fake quantization with the numerics of Int4Tensor (PLAIN packing): asymmetric, one scale and zero point per
    `group_size` weights along K (reference :81-101).  On MI355X: bf16 activations, the fake quantizer of Int4WeightOnlyConfig."""

    group_size: int = 128
    activation_dtype: torch.dtype = torch.bfloat16

    def __post_init__(self):
        if self.activation_dtype not in [e4m3_dtype, torch.bfloat16]:
            raise ValueError(f"Only {e4m3_dtype} or torch.bfloat16 activation are supported")
        if self.activation_dtype == e4m3_dtype:
            raise NotImplementedError(
                "Int4WeightFakeQuantizeConfig(activation_dtype=torch.float8_e4m3fn): the fake quantizer of "
                "Float8DynamicActivationInt4WeightConfig (a float8 rowwise pass, then symmetric int4) is not implemented on MI355X; use "
                "activation_dtype=torch.bfloat16, the fake quantizer of Int4WeightOnlyConfig")


def _infer_fake_quantize_configs(base_config: AOBaseConfig) -> Tuple[Optional[FakeQuantizeConfigBase], Optional[FakeQuantizeConfigBase]]:
    """(activation_config, weight_config) for a base post-training config, as the prepare step uses them (reference :345-489)."""
    if isinstance(base_config, Int4WeightOnlyConfig):
        if base_config.version != 2:
            raise ValueError(f"Unknown version on base config {type(base_config)}")
        supported_packing_formats = [Int4PackingFormat.PLAIN]  # (the reference also lists PRESHUFFLED, an H100 layout)
        if base_config.int4_packing_format not in supported_packing_formats:
            raise ValueError(f"Packing format must be one of {supported_packing_formats}")
        return None, Int4WeightFakeQuantizeConfig(group_size=base_config.group_size, activation_dtype=torch.bfloat16)
    if isinstance(base_config, Float8DynamicActivationFloat8WeightConfig):
        if base_config.version != 2:
            raise ValueError(f"Only version 2 of {type(base_config)} is supported")
        act_granularity, weight_granularity = base_config.granularity  # (normalised to a pair by the config itself)
        act_config = Float8FakeQuantizeConfig(dtype=base_config.activation_dtype, granularity=act_granularity,
                                              hp_value_lb=base_config.activation_value_lb, hp_value_ub=base_config.activation_value_ub)
        weight_config = Float8FakeQuantizeConfig(dtype=base_config.weight_dtype, granularity=weight_granularity)
        return act_config, weight_config
    raise ValueError("Unexpected base config: %s" % base_config)
