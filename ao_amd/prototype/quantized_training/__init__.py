"""Quantized training (torchao/prototype/quantized_training) on the MI355X.  Built: BitNet b1.58 (bitnet.py; csrc/bitnet_kernels.hip) and
int8 mixed precision (int8_mixed_precision.py, with int8.py's quantize_int8_rowwise; csrc/int8_train_kernels.hip).
Not built: the int8 quantized-training weight of int8.py (Int8QuantizedTrainingLinearWeight, Int8WeightOnlyQuantizedTrainingConfig)."""
from .bitnet import (  # noqa: F401
    BitNetInferenceConfig,
    BitNetPacked2bitLinearWeight,
    BitNetTrainingConfig,
    BitNetTrainingLinearWeight,
    _pack_i2_in_i8,
    _unpack_i2_in_i8,
    bitnet_training,
    get_bitnet_scale,
    precompute_bitnet_scale_for_fsdp,
    quantize_bitnet_weight,
)
from .int8 import quantize_int8_rowwise  # noqa: F401
from .int8_mixed_precision import (  # noqa: F401
    Int8MixedPrecisionTrainingConfig,
    Int8MixedPrecisionTrainingLinear,
    Int8MixedPrecisionTrainingLinearWeight,
    _dynamic_int8_mm,
    _Int8MixedPrecisionTrainingLinearFunction,
    int8_mixed_precision_training,
)

__all__ = ["BitNetTrainingConfig", "BitNetTrainingLinearWeight", "BitNetPacked2bitLinearWeight", "BitNetInferenceConfig", "bitnet_training",
           "get_bitnet_scale", "quantize_bitnet_weight", "precompute_bitnet_scale_for_fsdp", "quantize_int8_rowwise",
           "Int8MixedPrecisionTrainingConfig", "Int8MixedPrecisionTrainingLinear", "Int8MixedPrecisionTrainingLinearWeight",
           "int8_mixed_precision_training"]
