"""float8 training (torchao.float8), MI355X-native: the names torchao/float8/__init__.py exports that exist here.  Float8Linear and the
Function live in .float8_linear, as in the reference, where they are not public either."""
from .config import (
    CastConfig,
    Float8GemmConfig,
    Float8LinearConfig,
    Float8LinearRecipeName,
    ScalingGranularity,
    ScalingType,
    e4m3_dtype,
    e5m2_dtype,
)
from .float8_linear import Float8Linear, GemmInputRole, LinearMMConfig, ScaledMMConfig
from .float8_linear_utils import convert_to_float8_training

__all__ = [
    # configuration
    "ScalingType",
    "ScalingGranularity",
    "Float8GemmConfig",
    "Float8LinearConfig",
    "Float8LinearRecipeName",
    "CastConfig",
    "e4m3_dtype",
    "e5m2_dtype",
    # top level UX
    "convert_to_float8_training",
    # the per-GEMM config tuples of float8_training_tensor.py
    "GemmInputRole",
    "LinearMMConfig",
    "ScaledMMConfig",
    "Float8Linear",
]
