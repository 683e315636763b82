"""Prototype-namespace mirrors (torchao/prototype/*) that sit on the SURVEY.md section 8 path."""
from .awq import AWQConfig, AWQObservedLinear, AWQObserver  # noqa: F401
from .blockwise_fp8 import Float8BlockwiseExpertWeights, fp8_blockwise_grouped_mm  # noqa: F401
from .blockwise_fp8_grouped_training import (  # noqa: F401
    _Float8BlockwiseGroupedMM,
    _to_fp8_blockwise_then_emulated_scaled_grouped_mm,
    _to_fp8_blockwise_then_scaled_grouped_mm,
)
from .blockwise_fp8_training import Float8BlockwiseLinear, Float8BlockwiseLinearConfig, fp8_blockwise_mm  # noqa: F401
from .fp8_grouped_training import (  # noqa: F401
    Float8TrainingOpConfig,
    Float8TrainingRecipe,
    Float8TrainingWeightWrapperTensor,
    _Float8GroupedMM,
    _to_fp8_rowwise_then_scaled_grouped_mm,
)
from .gptq import GPTQConfig, GPTQObserverTensor, gptq_quantize  # noqa: F401
from .mx_training import (  # noqa: F401
    MXFP8Linear,
    MXFP8TrainingOpConfig,
    MXFP8TrainingRecipe,
    MXFP8TrainingWeightWrapperTensor,
    _to_mxfp8_then_scaled_mm,
    mx_mm,
)
from ..quantization.intx_tensor import IntxBitPackedTensor  # noqa: F401  (the device-packed sibling of IntxUnpackedToInt8Tensor)
from .codebook import (  # noqa: F401
    CodebookQuantizedTensor,
    CodebookWeightOnlyConfig,
    choose_qparams_codebook,
    codebook_weight_only,
    dequantize_codebook,
    quantize_codebook,
)
from .int4_opaque_tensor import Int4OpaqueTensor, Int8DynamicActivationInt4WeightConfig  # noqa: F401
from .nf4_api import NF4WeightOnlyConfig, nf4_weight_only  # noqa: F401
from .nvfp4_grouped import NVFP4ExpertWeights, nvfp4_grouped_mm  # noqa: F401
from .nvfp4_grouped_training import _NVFP4GroupedMM, _to_nvfp4_rht_rs_then_scaled_grouped_mm  # noqa: F401
from .nvfp4_tensor import (  # noqa: F401
    NVFP4DynamicActivationNVFP4WeightConfig,
    NVFP4Tensor,
    NVFP4WeightOnlyConfig,
    QuantizeTensorToNVFP4Kwargs,
    per_tensor_amax_to_scale,
)
from .nvfp4_training import (  # noqa: F401
    DEFAULT_SIGN_VECTOR,
    NVFP4Linear,
    NVFP4TrainingConfig,
    get_wgrad_sign_vector,
    nvfp4_linear,
)
from .attention import AttentionBackend, HadamardMode, apply_low_precision_attention, fp8_sdpa  # noqa: F401
from .smoothquant import (  # noqa: F401
    RunningAbsMaxSmoothQuantObserver,
    SmoothQuantConfig,
    SmoothQuantObservedLinear,
    SmoothQuantObserver,
    SmoothQuantStep,
)

__all__ = ["Float8BlockwiseExpertWeights", "fp8_blockwise_grouped_mm", "NVFP4Tensor", "NVFP4WeightOnlyConfig",
           "NVFP4DynamicActivationNVFP4WeightConfig", "QuantizeTensorToNVFP4Kwargs", "per_tensor_amax_to_scale", "NVFP4ExpertWeights",
           "nvfp4_grouped_mm", "MXFP8Linear", "MXFP8TrainingOpConfig", "MXFP8TrainingRecipe", "MXFP8TrainingWeightWrapperTensor",
           "_to_mxfp8_then_scaled_mm", "mx_mm", "Float8TrainingOpConfig", "Float8TrainingRecipe", "Float8TrainingWeightWrapperTensor",
           "_Float8GroupedMM", "_to_fp8_rowwise_then_scaled_grouped_mm", "fp8_blockwise_mm", "Float8BlockwiseLinear",
           "Float8BlockwiseLinearConfig", "_Float8BlockwiseGroupedMM", "_to_fp8_blockwise_then_scaled_grouped_mm",
           "_to_fp8_blockwise_then_emulated_scaled_grouped_mm",
           "NVFP4Linear", "NVFP4TrainingConfig", "nvfp4_linear", "DEFAULT_SIGN_VECTOR", "get_wgrad_sign_vector",
           "_NVFP4GroupedMM", "_to_nvfp4_rht_rs_then_scaled_grouped_mm",
           "NF4WeightOnlyConfig", "nf4_weight_only", "AWQConfig", "AWQObserver", "AWQObservedLinear",
           "SmoothQuantConfig", "SmoothQuantStep", "SmoothQuantObserver", "RunningAbsMaxSmoothQuantObserver", "SmoothQuantObservedLinear",
           "AttentionBackend", "HadamardMode", "apply_low_precision_attention", "fp8_sdpa",
           "IntxBitPackedTensor",
           "CodebookWeightOnlyConfig", "codebook_weight_only", "CodebookQuantizedTensor", "choose_qparams_codebook", "quantize_codebook",
           "dequantize_codebook", "Int4OpaqueTensor", "Int8DynamicActivationInt4WeightConfig"]
