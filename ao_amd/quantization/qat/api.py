"""QATConfig for quantize_ (reference: torchao/quantization/qat/api.py:33-307).

    quantize_(model, QATConfig(Int4WeightOnlyConfig(group_size=32), step="prepare"))   # nn.Linear -> FakeQuantizedLinear
    train(model)
    quantize_(model, QATConfig(Int4WeightOnlyConfig(group_size=32), step="convert"))   # -> nn.Linear with an Int4Tensor weight

nn.Embedding has no fake quantizer here.
"""
from enum import Enum
from typing import Optional

import torch

from ..config import AOBaseConfig
from ..quant_api import _QUANTIZE_CONFIG_HANDLER, register_quantize_module_handler
from .fake_quantize_config import FakeQuantizeConfigBase, _infer_fake_quantize_configs
from .linear import FakeQuantizedLinear


class QATStep(str, Enum):
    """The `step` of a QATConfig."""

    PREPARE = "prepare"
    CONVERT = "convert"


class QATConfig(AOBaseConfig):
    """Quantization-aware training through quantize_: "prepare" swaps every nn.Linear for a FakeQuantizedLinear, "convert" swaps it back
    and applies the base config.  Give either `base_config` (the fake quantizers are inferred from it; Int4WeightOnlyConfig with PLAIN
    packing and Float8DynamicActivationFloat8WeightConfig with PerRow() here) or the fake-quantize configs themselves."""

    def __init__(self, base_config: Optional[AOBaseConfig] = None, activation_config: Optional[FakeQuantizeConfigBase] = None,
                 weight_config: Optional[FakeQuantizeConfigBase] = None, *, step: QATStep = "prepare"):
        self.base_config = base_config
        self.activation_config = activation_config
        self.weight_config = weight_config
        self.step = step
        self.__post_init__()

    def __repr__(self):
        return (f"QATConfig(base_config={self.base_config!r}, activation_config={self.activation_config!r}, "
                f"weight_config={self.weight_config!r}, step={self.step!r})")

    def __post_init__(self):
        self.step = self.step.lower()
        all_step_values = [s.value for s in QATStep]
        if self.step not in all_step_values:
            raise ValueError(f"`step` must be one of {all_step_values}")
        if self.base_config is not None and self.activation_config is not None:
            raise ValueError("Cannot specify both `base_config` and `activation_config`")
        if self.base_config is not None and self.weight_config is not None:
            raise ValueError("Cannot specify both `base_config` and `weight_config`")
        if self.step == QATStep.PREPARE and not any((self.base_config, self.activation_config, self.weight_config)):
            raise ValueError("Must specify `base_config`, `activation_config`, or `weight_config` in the prepare step")
        if self.step == QATStep.CONVERT and (self.activation_config is not None or self.weight_config is not None):
            raise ValueError("Cannot specify `weight_config` or `activation_config` in the convert step")
        if isinstance(self.base_config, FakeQuantizeConfigBase):
            config_type = self.base_config.__class__.__name__
            raise ValueError(
                f"{config_type} was passed as `base_config`. Did you mean to do the following instead?\n"
                "    qat_config = QATConfig(\n"
                f"        activation_config={config_type}(...),\n"
                f"        weight_config={config_type}(...),\n"
                '        step="prepare",\n'
                "    )"
            )


@register_quantize_module_handler(QATConfig)
def _qat_config_transform(module: torch.nn.Module, config: QATConfig) -> torch.nn.Module:
    """prepare: nn.Linear -> FakeQuantizedLinear over the same parameters.  convert: FakeQuantizedLinear -> nn.Linear, then the base
    config's own handler; other modules pass through."""
    base_config = config.base_config
    if config.step == QATStep.PREPARE:
        if base_config is not None:
            act_config, weight_config = _infer_fake_quantize_configs(base_config)
        else:
            act_config, weight_config = config.activation_config, config.weight_config
        if isinstance(module, torch.nn.Linear):
            return FakeQuantizedLinear.from_linear(module, act_config, weight_config)
        raise ValueError("Module of type '%s' does not have QAT support" % type(module))
    assert config.step == QATStep.CONVERT, "unexpected step '%s' in QATConfig" % config.step
    assert config.activation_config is None, "unexpected `activation_config`"
    assert config.weight_config is None, "unexpected `weight_config`"
    if not isinstance(module, FakeQuantizedLinear):
        return module
    module = module.to_linear()
    if base_config is None:
        return module
    return _QUANTIZE_CONFIG_HANDLER[type(base_config)](module, base_config)
