"""SmoothQuant for MI355X: SmoothQuantConfig and its quantize_ handler.

Host-side mirror of torchao/prototype/smoothquant/api.py (same public names, same steps):

    base = Int8DynamicActivationInt8WeightConfig()                           # or Int8StaticActivationInt8WeightConfig(granularity=PerTensor())
    quantize_(model, SmoothQuantConfig(base, step="prepare", alpha=0.5))     # every nn.Linear becomes a SmoothQuantObservedLinear
    for batch in calibration: model(batch)                                   # every forward folds its input into a running [K] maximum
    quantize_(model, SmoothQuantConfig(base, step="convert", alpha=0.5))     # nn.Linear, Int8Tensor weight, act_pre_scale = 1 / factor
    quantize_(fresh, SmoothQuantConfig(base, step="prepare_for_loading"))    # the same tensor fields without calibration, to load into

  and with use_running_absmax=True the two-pass flow: prepare, calibrate, step="prepare_for_smoothquant_smoothing_factor", calibrate again,
  convert.

SmoothQuant (https://arxiv.org/abs/2211.10438) moves activation outliers into the weight: input channel k of the weight is multiplied by
s[k] = max|x_k|^alpha / max|w_k|^(1 - alpha) before it is quantized and the activation is divided by s[k] at run time.  The product is the
existing Int8Tensor with act_pre_scale = 1 / s; its F.linear folds the pre-scale into the activation cast (quantization/int8_tensor.py
_prescale_fuses, csrc/quant_kernels.hip).

Deviations, on purpose:
  * SmoothQuantStep: the reference adds prepare_for_smoothquant_smoothing_factor / _activation_scales to QuantizationStep; here that enum
    keeps its three members and this package defines the five-member SmoothQuantStep.  `step` takes either enum or a string.
  * prepare_for_loading runs NO calibration (the reference calibrates on one random row): the weight goes through the base handler with
    act_pre_scale = ones(K) and, for a static base config, a placeholder act_quant_scale of one element.
  * the base config is not modified: the calibrated act_quant_scale goes into a copy.

Supported: Int8DynamicActivationInt8WeightConfig (any granularity pair and activation mapping it accepts) and
Int8StaticActivationInt8WeightConfig with a PerTensor symmetric activation and a PerRow or PerTensor weight, on bfloat16 2-D weights with
K % 8 == 0.  Everything else is refused by name, at `prepare`, before any calibration is spent.
"""
import dataclasses
import enum
import logging
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from ...quantization.config import AOBaseConfig, Int8DynamicActivationInt8WeightConfig, Int8StaticActivationInt8WeightConfig
from ...quantization.granularity import PerRow, PerTensor
from ...quantization.quant_api import _QUANTIZE_CONFIG_HANDLER, _set_weight_only, register_quantize_module_handler
from ...quantization.quant_primitives import MappingType
from ..nvfp4_tensor import QuantizationStep
from .core import RunningAbsMaxSmoothQuantObserver, SmoothQuantObservedLinear, SmoothQuantObserver

__all__ = ["SmoothQuantConfig", "SmoothQuantStep"]

logger = logging.getLogger(__name__)

_SUPPORTED = ("SmoothQuant on MI355X supports Int8DynamicActivationInt8WeightConfig and Int8StaticActivationInt8WeightConfig with a PerTensor "
              "symmetric activation (weights PerRow or PerTensor), on bfloat16 2-D weights whose K is a multiple of 8")


class SmoothQuantStep(str, enum.Enum):
    """The reference's QuantizationStep with its two SmoothQuant members (quantize_/common/quantization_step.py)."""
    PREPARE = "prepare"
    CONVERT = "convert"
    PREPARE_FOR_LOADING = "prepare_for_loading"
    PREPARE_FOR_SMOOTHQUANT_SMOOTHING_FACTOR = "prepare_for_smoothquant_smoothing_factor"
    PREPARE_FOR_SMOOTHQUANT_ACTIVATION_SCALES = "prepare_for_smoothquant_activation_scales"


@dataclass
class SmoothQuantConfig(AOBaseConfig):
    """reference api.py:32-61 (same fields and defaults).

    base_config: the quantization SmoothQuant is applied on top of.
    step: a SmoothQuantStep, a QuantizationStep, or the string of either, any letter case.
    alpha: the exponent of the smoothing factor; None gives a factor of ones (plain quantization).
    use_running_absmax: use RunningAbsMaxSmoothQuantObserver and its two calibration passes."""

    base_config: AOBaseConfig
    step: SmoothQuantStep
    alpha: Optional[float] = 0.5
    use_running_absmax: bool = False

    def __post_init__(self):
        self.step = self.step.lower() if isinstance(self.step, str) and not isinstance(self.step, enum.Enum) else self.step.value
        all_step_values = [s.value for s in SmoothQuantStep]
        if self.step not in all_step_values:
            raise ValueError(f"{self.step} is not one of {all_step_values}")


def _is_static(base_config) -> bool:
    return isinstance(base_config, Int8StaticActivationInt8WeightConfig)


def _check_base_config(base_config):
    """A supported base_config passes; everything else is refused by name."""
    if isinstance(base_config, Int8DynamicActivationInt8WeightConfig):
        return
    if _is_static(base_config):
        act_granularity = base_config.granularity[0]
        if isinstance(act_granularity, PerRow):
            raise NotImplementedError("SmoothQuant on MI355X: a static PerRow activation (Int8StaticActivationInt8WeightConfig with granularity "
                                      f"{base_config.granularity}) is not implemented: its scale has one entry per calibration row, which only "
                                      f"fits an input of the calibration's shape.  Use granularity=PerTensor() or [PerTensor(), PerRow()].  {_SUPPORTED}")
        if not isinstance(act_granularity, PerTensor):
            raise NotImplementedError(f"SmoothQuant on MI355X: static activation granularity {act_granularity} is not implemented.  {_SUPPORTED}")
        if base_config.act_mapping_type != MappingType.SYMMETRIC:
            raise NotImplementedError("SmoothQuant on MI355X: a static ASYMMETRIC activation (Int8StaticActivationInt8WeightConfig with "
                                      f"act_mapping_type {base_config.act_mapping_type}) is not implemented.  {_SUPPORTED}")
        return
    raise NotImplementedError(f"SmoothQuant on MI355X: unsupported base_config {type(base_config).__name__}.  {_SUPPORTED}")


def _check_weight(W):
    if W.dim() != 2:
        raise NotImplementedError(f"SmoothQuant quantizes 2-D weights, got shape {tuple(W.shape)}.  {_SUPPORTED}")
    if W.dtype != torch.bfloat16:
        raise NotImplementedError(f"SmoothQuant on MI355X takes bfloat16 weights, got {W.dtype}.  {_SUPPORTED}")
    if W.shape[1] == 0 or W.shape[1] % 8 != 0:
        raise NotImplementedError(f"SmoothQuant on MI355X: K={W.shape[1]} is not a multiple of 8.  {_SUPPORTED}")


class _WeightHolder(nn.Module):
    """What the base handler quantizes: a module with a `weight` (the reference's DummyModule)."""

    def __init__(self, weight):
        super().__init__()
        self.weight = weight


def _quantized_linear(module, base_config, weight, act_pre_scale, act_quant_scale):
    """A fresh nn.Linear whose weight is base_handler(weight) with act_pre_scale set, and the module's bias (reference api.py:133-164)."""
    if _is_static(base_config):
        base_config = dataclasses.replace(base_config, act_quant_scale=act_quant_scale, act_quant_zero_point=None)
    qw = _QUANTIZE_CONFIG_HANDLER[type(base_config)](_WeightHolder(nn.Parameter(weight, requires_grad=False)), base_config).weight
    qw = qw.detach()
    assert hasattr(qw, "act_pre_scale"), "weight must support activation pre-scaling (an `act_pre_scale` attribute)"
    qw.act_pre_scale = act_pre_scale
    linear = nn.Linear(module.in_features, module.out_features, False, device="meta", dtype=module.weight.dtype)
    _set_weight_only(linear, "weight", qw)
    linear.bias = module.bias
    return linear


@register_quantize_module_handler(SmoothQuantConfig)
def _smooth_quant_transform(module: nn.Module, config: SmoothQuantConfig, *, parameter_name="weight") -> nn.Module:
    """reference api.py:64-164"""
    if parameter_name != "weight":
        raise NotImplementedError(f"SmoothQuant on MI355X quantizes the `weight` of a linear, got parameter {parameter_name!r}")
    step, base_config = config.step, config.base_config
    observed = isinstance(module, SmoothQuantObservedLinear)

    if step == SmoothQuantStep.PREPARE_FOR_SMOOTHQUANT_SMOOTHING_FACTOR:
        if observed and isinstance(module.obs, RunningAbsMaxSmoothQuantObserver):
            module.obs.compute_smoothing_factor()
        return module
    if step == SmoothQuantStep.PREPARE_FOR_SMOOTHQUANT_ACTIVATION_SCALES:
        return module  # reserved for future use (reference api.py:115-117)
    if step == SmoothQuantStep.CONVERT and not observed:
        logger.info(f"convert: module is not SmoothQuantObservedLinear, skipping: {type(module)}")
        return module

    _check_base_config(base_config)  # an unsupported target is refused before any calibration is spent on it
    W = module.weight.detach()
    _check_weight(W)

    if step == SmoothQuantStep.PREPARE:
        if config.use_running_absmax:
            observer = RunningAbsMaxSmoothQuantObserver(weight=module.weight, alpha=config.alpha)
        else:
            observer = SmoothQuantObserver(weight=module.weight, alpha=config.alpha, keep_inputs=_is_static(base_config))
        return SmoothQuantObservedLinear.from_float(module, observer)
    if step == SmoothQuantStep.PREPARE_FOR_LOADING:
        ones = torch.ones(W.shape[1], dtype=W.dtype, device=W.device)
        placeholder = None
        if _is_static(base_config):  # the shape a converted model's scale has: [1, 1] from the default observer, 0-dim from the running one
            placeholder = torch.ones(() if config.use_running_absmax else (1, 1), dtype=torch.float32, device=W.device)
        return _quantized_linear(module, base_config, W.contiguous(), ones, placeholder)
    assert step == SmoothQuantStep.CONVERT, f"Unexpected step: {step}"
    quant_kwargs = base_config.get_act_quant_kwargs() if _is_static(base_config) else None
    smoothing_factor, activation_scale, activation_zero_point = module.obs.calculate_qparams(weight_quant_kwargs=quant_kwargs)
    if _is_static(base_config) and activation_scale is None:
        raise RuntimeError("SmoothQuant convert: the running observer has no activation scale yet: run the step "
                           "'prepare_for_smoothquant_smoothing_factor' and a second calibration pass before convert")
    module.obs.release()
    # the activation is multiplied by act_pre_scale at run time, so the reciprocal of the smoothing factor is what is saved
    return _quantized_linear(module, base_config, (W * smoothing_factor).contiguous(), 1.0 / smoothing_factor, activation_scale)
