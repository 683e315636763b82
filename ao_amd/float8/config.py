"""Configuration of float8 training: the host mirror of torchao/float8/config.py:19-381.

Field names, defaults and the checks of `__post_init__` are the reference's, so that a config written for it is read here unchanged;
the dataclasses are frozen like its own.  What this backend runs of it is decided where a config is USED (float8_linear.py:
`check_config`), not here: the constructors accept everything the reference's accept, e5m2 gradients included.

gfx950 implements the OCP formats, so `e4m3_dtype` / `e5m2_dtype` are torch.float8_e4m3fn / torch.float8_e5m2 (config.py:66-89 picks the
fnuz pair on MI300 only).
"""
import enum
import logging
from dataclasses import dataclass
from typing import Optional, Union

import torch

logger = logging.getLogger()

e4m3_dtype = torch.float8_e4m3fn
e5m2_dtype = torch.float8_e5m2


class ScalingType(enum.Enum):
    """How a tensor is scaled for its cast (config.py:19-39): DYNAMIC from its own values, DISABLED leaves it in high precision."""

    DYNAMIC = "dynamic"
    DISABLED = "disabled"

    def short_str(self):
        return {ScalingType.DYNAMIC: "dyn", ScalingType.DISABLED: "dis"}[self]


class ScalingGranularity(enum.Enum):
    """One scale for the tensor, or one per slice along an axis (config.py:42-63)."""

    TENSORWISE = "tensorwise"
    AXISWISE = "axiswise"

    def short_str(self):
        return {ScalingGranularity.TENSORWISE: "ten", ScalingGranularity.AXISWISE: "axs"}[self]


@dataclass(frozen=True)
class CastConfig:
    """The cast of one tensor (config.py:92-121).  target_dtype None: filled in by Float8LinearConfig (e4m3 for input and weight, e5m2
    for grad_output)."""

    scaling_type: ScalingType = ScalingType.DYNAMIC
    scaling_granularity: ScalingGranularity = ScalingGranularity.TENSORWISE
    target_dtype: Optional[torch.dtype] = None

    def short_str(self):
        dtype = {e4m3_dtype: "e4m3", e5m2_dtype: "e5m2"}[self.target_dtype]
        return f"{self.scaling_type.short_str()}_{self.scaling_granularity.short_str()}_{dtype}"

    def __post_init__(self):
        if self.scaling_granularity is ScalingGranularity.AXISWISE:
            assert self.scaling_type is ScalingType.DYNAMIC, "only dynamic scaling type is supported for axiswise scaling granularity"
        assert self.target_dtype is None or (self.target_dtype.is_floating_point and self.target_dtype.itemsize == 1), (
            "must specify a 8-bit floating-point dtype")


@dataclass(frozen=True)
class Float8GemmConfig:
    """One of the three GEMMs (config.py:124-137).  use_fast_accum is accepted and selects nothing on gfx950: the MFMA accumulates in
    fp32 either way."""

    use_fast_accum: bool = False


class Float8LinearRecipeName(enum.Enum):
    """The pre-made recipes (config.py:140-176)."""

    TENSORWISE = "tensorwise"
    ROWWISE = "rowwise"
    ROWWISE_WITH_GW_HP = "rowwise_with_gw_hp"


@dataclass(frozen=True)
class Float8LinearConfig:
    """How an nn.Linear trains in float8 (config.py:179-381): a CastConfig for each of input, weight and grad_output, with an optional
    second one for the other GEMM the tensor is an operand of (None: the same), a Float8GemmConfig per GEMM, and the per-linear flags."""

    cast_config_input: CastConfig = CastConfig()
    cast_config_input_for_grad_weight: Optional[CastConfig] = None
    cast_config_weight: CastConfig = CastConfig()
    cast_config_weight_for_grad_input: Optional[CastConfig] = None
    cast_config_grad_output: CastConfig = CastConfig()
    cast_config_grad_output_for_grad_weight: Optional[CastConfig] = None

    gemm_config_output: Float8GemmConfig = Float8GemmConfig(use_fast_accum=True)
    gemm_config_grad_input: Float8GemmConfig = Float8GemmConfig()
    gemm_config_grad_weight: Float8GemmConfig = Float8GemmConfig()

    enable_fsdp_float8_all_gather: bool = False
    pad_inner_dim: bool = False
    emulate: bool = False
    force_recompute_fp8_weight_in_bwd: bool = False
    round_scales_to_power_of_2: bool = False

    def __post_init__(self):
        # the dataclass is frozen for its users; its own defaults are filled in through object.__setattr__, as in the reference
        for second, first in (("cast_config_input_for_grad_weight", "cast_config_input"),
                              ("cast_config_weight_for_grad_input", "cast_config_weight"),
                              ("cast_config_grad_output_for_grad_weight", "cast_config_grad_output")):
            if getattr(self, second) is None:
                object.__setattr__(self, second, getattr(self, first))

        if self.cast_config_weight.scaling_granularity != ScalingGranularity.TENSORWISE:
            assert not self.enable_fsdp_float8_all_gather, (
                f"enable_fsdp_float8_all_gather only supports tensorwise scaling granularity, got {self.cast_config_weight.scaling_granularity}")

        cc_i, cc_w, cc_go = self.cast_config_input, self.cast_config_weight, self.cast_config_grad_output
        cc_i_gw, cc_w_gi = self.cast_config_input_for_grad_weight, self.cast_config_weight_for_grad_input
        cc_go_gw = self.cast_config_grad_output_for_grad_weight
        # a GEMM takes both operands in float8 or both in high precision
        for a, b, gemm_name in ((cc_i, cc_w, "output"), (cc_go, cc_w_gi, "grad_input"), (cc_i_gw, cc_go_gw, "grad_weight")):
            assert (a.scaling_type is ScalingType.DISABLED) == (b.scaling_type is ScalingType.DISABLED), (
                f"incompatible operand precision for {gemm_name}")

        for a, b, operand_name, default_dtype in ((cc_i, cc_i_gw, "input", e4m3_dtype), (cc_w, cc_w_gi, "weight", e4m3_dtype),
                                                  (cc_go, cc_go_gw, "grad_output", e5m2_dtype)):
            for cc in (a, b):
                if cc.target_dtype is None:
                    object.__setattr__(cc, "target_dtype", default_dtype)
            assert a.target_dtype == b.target_dtype, f"{operand_name} must be cast to the same dtype in both matmuls it's used in"

        if self.force_recompute_fp8_weight_in_bwd:
            logger.warning("`config.force_recompute_fp8_weight_in_bwd` is deprecated and has no effect")

    @staticmethod
    def from_recipe_name(recipe_name: Union[Float8LinearRecipeName, str]) -> "Float8LinearConfig":
        """The config of a recipe, by enum value or by its string (config.py:316-381)."""
        if type(recipe_name) == str:
            valid_names = [n.value for n in Float8LinearRecipeName]
            assert recipe_name in valid_names, f"recipe_name {recipe_name} not in valid names {valid_names}"
            recipe_name = Float8LinearRecipeName(recipe_name)

        axiswise = ScalingGranularity.AXISWISE
        if recipe_name is Float8LinearRecipeName.TENSORWISE:
            return Float8LinearConfig()
        if recipe_name is Float8LinearRecipeName.ROWWISE:
            # e4m3 everywhere, one scale per row of each GEMM operand, scales rounded down to powers of two
            return Float8LinearConfig(
                cast_config_input=CastConfig(scaling_granularity=axiswise, target_dtype=e4m3_dtype),
                cast_config_weight=CastConfig(scaling_granularity=axiswise, target_dtype=e4m3_dtype),
                cast_config_grad_output=CastConfig(scaling_granularity=axiswise, target_dtype=e4m3_dtype),
                round_scales_to_power_of_2=True,
            )
        if recipe_name is Float8LinearRecipeName.ROWWISE_WITH_GW_HP:
            # output: axiswise x axiswise;  grad_input: grad_output axiswise x weight tensorwise;  grad_weight: in high precision
            return Float8LinearConfig(
                cast_config_input=CastConfig(scaling_granularity=axiswise),
                cast_config_weight=CastConfig(scaling_granularity=axiswise),
                cast_config_grad_output=CastConfig(scaling_granularity=axiswise, target_dtype=e4m3_dtype),
                cast_config_input_for_grad_weight=CastConfig(scaling_type=ScalingType.DISABLED),
                cast_config_weight_for_grad_input=CastConfig(scaling_granularity=ScalingGranularity.TENSORWISE),
                cast_config_grad_output_for_grad_weight=CastConfig(scaling_type=ScalingType.DISABLED, target_dtype=e4m3_dtype),
                round_scales_to_power_of_2=True,
            )
        raise AssertionError(f"unknown recipe_name {recipe_name}")
