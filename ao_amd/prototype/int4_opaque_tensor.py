"""W4A8 weights (reference: torchao/prototype/quantization/int4/int4_opaque_tensor.py and inference_workflow.py).

Int4OpaqueTensor carries the reference's field names over this library's own packed layout (the reference's is VNNI-blocked for its
CPU kernel and "opaque" by name): qdata int32 [N, Kp / 8], scale_and_zero float32 [G, N, 2] (what the kernels read), qzeros int8 [G, N],
compensation int16 [G, N] (csrc/da8w4_kernels.hip states the layout and the arithmetic).  from_hp_da8w4 is ONE launch, F.linear is two:
the per-token int8 cast of the activation and the int8 x int4 GEMM with an exact int32 sum per group (ops.da8w4_linear).

Only the DA8W4 half of the reference's tensor is built: its A16W4 from_hp packs for the CPU tinygemm kernel and is refused by name."""
import logging
from dataclasses import dataclass
from typing import List

import torch
import torch.nn.functional as F

from .. import ops
from ..quantization.base_tensor import LowBitTensorBase
from ..quantization.config import AOBaseConfig
from ..quantization.quant_api import register_quantize_module_handler
from ..quantization.quant_primitives import MappingType

aten = torch.ops.aten
logger = logging.getLogger(__name__)


class Int4OpaqueTensor(LowBitTensorBase):
    """qdata, scale_and_zero, qzeros, compensation; attributes block_size [1, group_size], shape [N, K], act_mapping_type
    ("asymmetric" / "symmetric")."""

    tensor_data_names = ["qdata", "scale_and_zero", "qzeros", "compensation"]
    tensor_attribute_names = ["block_size", "shape", "act_mapping_type"]

    def __new__(cls, qdata, scale_and_zero, qzeros, compensation, block_size, shape, act_mapping_type):
        return torch.Tensor._make_wrapper_subclass(cls, shape, device=qdata.device, dtype=torch.bfloat16, requires_grad=False)

    def __init__(self, qdata, scale_and_zero, qzeros, compensation, block_size, shape, act_mapping_type):
        assert act_mapping_type in ("asymmetric", "symmetric"), f"act_mapping_type must be asymmetric or symmetric, got {act_mapping_type!r}"
        self.qdata, self.scale_and_zero, self.qzeros, self.compensation = qdata, scale_and_zero, qzeros, compensation
        self.block_size = list(block_size)
        self.act_mapping_type = act_mapping_type

    def _quantization_type(self):
        return f"da8w4, shape={tuple(self.shape)}, block_size={self.block_size}, act={self.act_mapping_type}, device={self.device}"

    @classmethod
    def from_hp(cls, w: torch.Tensor, block_size: List[int], int4_choose_qparams_algorithm=None):
        raise NotImplementedError("Int4OpaqueTensor.from_hp (A16W4) packs for the CPU tinygemm kernel and is not built on MI355X: use "
                                  "Int4WeightOnlyConfig for bf16 activations x int4 weights, or from_hp_da8w4 for int8 activations")

    @classmethod
    def from_hp_da8w4(cls, w: torch.Tensor, group_size: int = 32, act_mapping_type: MappingType = MappingType.ASYMMETRIC):
        """reference :214-291: asymmetric 4-bit codes per group, packed with the scales, zero-points and compensation in one launch"""
        assert w.ndim == 2, f"Expecting 2D tensor, but got: {tuple(w.shape)}"
        assert group_size in ops.DA8W4_GROUP_SIZES, f"Expecting group_size to be 32/64/128, but got: {group_size}"
        assert w.shape[1] % group_size == 0, f"K={w.shape[1]} must be divisible by group_size={group_size}"
        assert w.shape[0] % 32 == 0, f"N={w.shape[0]} must be divisible by 32 for DA8W4"
        act_mapping_type = MappingType(act_mapping_type)
        assert act_mapping_type in (MappingType.ASYMMETRIC, MappingType.SYMMETRIC), f"act_mapping_type must be ASYMMETRIC or SYMMETRIC, got {act_mapping_type}"
        qdata, sz, qzeros, comp = ops.da8w4_quantize_weight(w.detach(), group_size)
        return cls(qdata, sz, qzeros, comp, [1, group_size], w.shape, "symmetric" if act_mapping_type == MappingType.SYMMETRIC else "asymmetric")

    def dequantize(self):
        """bf16((q - zero_point) * scale), exact, one launch"""
        return ops.da8w4_dequantize(self.qdata, self.scale_and_zero, self.shape[1])


@Int4OpaqueTensor.implements(aten.linear.default)
@Int4OpaqueTensor.implements_torch_function(F.linear)
def _(func, types, args, kwargs):
    x, w = args[0], args[1]
    bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
    if not isinstance(w, Int4OpaqueTensor) or isinstance(x, Int4OpaqueTensor):
        raise NotImplementedError("F.linear: only a plain activation with an Int4OpaqueTensor weight is built")
    if not x.is_cuda:
        raise RuntimeError("Int4OpaqueTensor: F.linear runs on the MI355X only; there is no CPU fallback")
    return ops.da8w4_linear(x, w.qdata, w.scale_and_zero, bias, symmetric=w.act_mapping_type == "symmetric")


@dataclass
class Int8DynamicActivationInt4WeightConfig(AOBaseConfig):
    """reference inference_workflow.py:92-121: group_size in {32, 64, 128}; act_mapping_type ASYMMETRIC (uint8 codes) or SYMMETRIC"""

    group_size: int = 32
    act_mapping_type: MappingType = MappingType.ASYMMETRIC
    set_inductor_config: bool = True  # (kept for the reference's signature; nothing here goes through inductor)


@register_quantize_module_handler(Int8DynamicActivationInt4WeightConfig)
def _int8_dynamic_act_int4_weight_transform(module: torch.nn.Module, config: Int8DynamicActivationInt4WeightConfig, *,
                                            parameter_name: str = "weight"):
    """reference :124-163, with its rule that a weight the format does not take is left untouched"""
    assert hasattr(module, parameter_name), f"applying DA8W4 quant requires module to have {parameter_name} attribute but {module} does not have one"
    weight = getattr(module, parameter_name)
    if weight.shape[-1] % config.group_size != 0 or config.group_size not in ops.DA8W4_GROUP_SIZES:
        logger.info(f"Skipping DA8W4 quantization: weight shape {weight.shape} is not compatible with group_size {config.group_size} "
                    "(must be divisible and one of [128, 64, 32])")
        return module
    if weight.shape[0] % 32 != 0:
        logger.info(f"Skipping DA8W4 quantization: weight shape {weight.shape} requires N divisible by 32")
        return module
    new_weight = Int4OpaqueTensor.from_hp_da8w4(weight, group_size=config.group_size, act_mapping_type=config.act_mapping_type)
    setattr(module, parameter_name, torch.nn.Parameter(new_weight, requires_grad=False))
    return module


torch.serialization.add_safe_globals([Int4OpaqueTensor])
