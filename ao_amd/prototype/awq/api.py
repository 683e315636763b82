"""AWQ for MI355X: AWQConfig and its quantize_ handler.

Host-side mirror of torchao/prototype/awq/api.py (same public names, same three steps):

    base = Int4WeightOnlyConfig(group_size=128, int4_packing_format="plain")
    quantize_(model, AWQConfig(base, step="prepare"))              # every nn.Linear becomes an AWQObservedLinear
    for batch in calibration: model(batch)                         # every forward folds its input into the observer's sums
    quantize_(model, AWQConfig(base, step="convert"))              # nn.Linear with an Int4Tensor weight, act_pre_scale = 1 / s
    quantize_(fresh, AWQConfig(base, step="prepare_for_loading"))  # the same tensor fields without calibration, to load a checkpoint into

AWQ (https://arxiv.org/abs/2306.00978) scales every input channel of the weight by s[k] before quantizing it and divides the activation by
s[k] at run time, s = mean|x|^ratio for the ratio in {0, 1/R, ..} whose quantized linear is closest to the original on the calibration
inputs.  The search is core.AWQObserver's (one launch and one matmul per chunk of ratios, csrc/awq_kernels.hip); the product is the existing
Int4Tensor with act_pre_scale set, which its F.linear multiplies into the activation.

Deviation, on purpose: prepare_for_loading runs NO search.  The reference calibrates on one random row and runs the whole
search only to get a tensor with the right fields (api.py:75-89); here the weight is Int4Tensor.from_hp(W) with act_pre_scale = ones(K): the
state dict has the keys, shapes and dtypes of a converted model's.  The other deviations are the observer's (core.py).

Supported: Int4WeightOnlyConfig with int4_packing_format PLAIN and the tinygemm (min / max) qparams, group sizes 32, 64, 128, 256, bfloat16
2-D weights whose K the group size divides.  Everything else is refused by name, at `prepare`, before any calibration is spent.
"""
import logging
from dataclasses import dataclass

import torch
import torch.nn as nn

from ... import ops
from ...quantization.config import (
    AOBaseConfig,
    Float8DynamicActivationInt4WeightConfig,
    Int4ChooseQParamsAlgorithm,
    Int4PackingFormat,
    Int4WeightOnlyConfig,
)
from ...quantization.quant_api import _set_weight_only, register_quantize_module_handler
from ..nvfp4_tensor import QuantizationStep
from .core import AWQObservedLinear, AWQObserver

__all__ = ["AWQConfig"]

logger = logging.getLogger(__name__)

_SUPPORTED = ("AWQ on MI355X supports Int4WeightOnlyConfig(int4_packing_format='plain') with the tinygemm (min / max) qparams, group_size 32, "
              "64, 128 or 256, on bfloat16 2-D weights whose K the group size divides")


@dataclass
class AWQConfig(AOBaseConfig):
    """reference api.py:30-54 (same fields and defaults).

    base_config: the quantization AWQ is applied on top of: Int4WeightOnlyConfig, PLAIN packing.
    step: "prepare" inserts the observers, "convert" turns the observed linears into linears with AWQ-scaled Int4Tensor weights,
        "prepare_for_loading" turns a float model into one with the same tensor fields, to load a converted model's state dict into.
        A QuantizationStep or its string, any letter case.
    scale_search_space_size: the number R of ratios i / R the search tries."""

    base_config: AOBaseConfig
    step: QuantizationStep
    scale_search_space_size: int = 20

    def __post_init__(self):
        self.step = (self.step.value if isinstance(self.step, QuantizationStep) else self.step).lower()
        all_step_values = [s.value for s in QuantizationStep]
        if self.step not in all_step_values:
            raise ValueError(f"{self.step} is not one of {all_step_values}")


def _group_size_of(base_config) -> int:
    """The group size of a supported base_config; everything else is refused by name."""
    if isinstance(base_config, Float8DynamicActivationInt4WeightConfig):
        raise NotImplementedError("AWQ on MI355X: the fp8-activation (symmetric) int4 flavour (Float8DynamicActivationInt4WeightConfig) is not "
                                  f"implemented; the search judges the zero-point quantizer of Int4WeightOnlyConfig.  {_SUPPORTED}")
    if isinstance(base_config, Int4WeightOnlyConfig):
        if base_config.int4_packing_format != Int4PackingFormat.PLAIN:
            raise NotImplementedError(f"AWQ on MI355X produces Int4Tensor (int4_packing_format PLAIN) only, got "
                                      f"{base_config.int4_packing_format.value!r}.  {_SUPPORTED}")
        if base_config.int4_choose_qparams_algorithm == Int4ChooseQParamsAlgorithm.HQQ:
            raise NotImplementedError(f"AWQ on MI355X: the HQQ qparams algorithm is not implemented.  {_SUPPORTED}")
        if base_config.group_size not in ops.AWQ_GROUP_SIZES:
            raise NotImplementedError(f"AWQ on MI355X: group_size {base_config.group_size} is not implemented.  {_SUPPORTED}")
        return base_config.group_size
    raise NotImplementedError(f"AWQ on MI355X: unsupported base_config {type(base_config).__name__}.  {_SUPPORTED}")


def _check_weight(W, group_size):
    if W.dim() == 3:
        raise NotImplementedError(f"AWQ on MI355X: 3-D expert weights are not implemented, got shape {tuple(W.shape)}.  {_SUPPORTED}")
    if W.dim() != 2:
        raise NotImplementedError(f"AWQ quantizes 2-D weights, got shape {tuple(W.shape)}.  {_SUPPORTED}")
    if W.dtype != torch.bfloat16:
        raise NotImplementedError(f"AWQ on MI355X takes bfloat16 weights, got {W.dtype}.  {_SUPPORTED}")
    if W.shape[1] == 0 or W.shape[1] % group_size != 0:
        raise NotImplementedError(f"AWQ on MI355X: K={W.shape[1]} is not a multiple of group_size={group_size}.  {_SUPPORTED}")


def _int4_linear(module, qw):
    """A fresh nn.Linear that carries the quantized weight and the module's bias (reference api.py:113-123)."""
    linear = nn.Linear(module.in_features, module.out_features, False, device="meta", dtype=module.weight.dtype)
    _set_weight_only(linear, "weight", qw)
    linear.bias = module.bias
    return linear


@register_quantize_module_handler(AWQConfig)
def _awq_transform(module: nn.Module, config: AWQConfig, *, parameter_name="weight") -> nn.Module:
    """reference api.py:57-123"""
    from ...quantization.int4_plain_tensor import Int4Tensor

    if parameter_name != "weight":
        raise NotImplementedError(f"AWQ on MI355X quantizes the `weight` of a linear, got parameter {parameter_name!r}")
    step = config.step
    if step == QuantizationStep.CONVERT and not isinstance(module, AWQObservedLinear):
        logger.info(f"convert: module is not AWQObservedLinear, skipping: {type(module)}")
        return module
    g = _group_size_of(config.base_config)  # an unsupported target is refused before any calibration is spent on it
    W = module.weight.detach()
    _check_weight(W, g)

    if step == QuantizationStep.PREPARE:
        observer = AWQObserver(module.weight, module.bias, config.base_config, config.scale_search_space_size)
        return AWQObservedLinear.from_float(module, observer)
    if step == QuantizationStep.PREPARE_FOR_LOADING:
        qw = Int4Tensor.from_hp(W.contiguous(), [1, g])
        qw.act_pre_scale = torch.ones(W.shape[1], dtype=W.dtype, device=W.device)
        return _int4_linear(module, qw)
    assert step == QuantizationStep.CONVERT, f"Unexpected step: {step}"
    equalization_scale = module.act_obs.calculate_qparams()
    module.act_obs.release()
    qw = Int4Tensor.from_hp((W * equalization_scale).contiguous(), [1, g])
    # the activation is multiplied by act_pre_scale at run time, so the reciprocal of the equalization scale is what is saved
    qw.act_pre_scale = 1.0 / equalization_scale
    return _int4_linear(module, qw)
