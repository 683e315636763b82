"""Quantized training (torchao/prototype/quantized_training) on the MI355X.  Built: BitNet b1.58 (bitnet.py; csrc/bitnet_kernels.hip).
Not built: the int8 quantized-training weight (int8.py) and int8 mixed precision (int8_mixed_precision.py)."""
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

__all__ = ["BitNetTrainingConfig", "BitNetTrainingLinearWeight", "BitNetPacked2bitLinearWeight", "BitNetInferenceConfig", "bitnet_training",
           "get_bitnet_scale", "quantize_bitnet_weight", "precompute_bitnet_scale_for_fsdp"]
