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
from .nf4_api import NF4WeightOnlyConfig, nf4_weight_only  # noqa: F401
from .nvfp4_grouped import NVFP4ExpertWeights, nvfp4_grouped_mm  # noqa: F401
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
           "NF4WeightOnlyConfig", "nf4_weight_only", "AWQConfig", "AWQObserver", "AWQObservedLinear",
           "SmoothQuantConfig", "SmoothQuantStep", "SmoothQuantObserver", "RunningAbsMaxSmoothQuantObserver", "SmoothQuantObservedLinear"]
