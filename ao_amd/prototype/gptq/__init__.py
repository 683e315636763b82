"""GPTQ (torchao/prototype/gptq): Hessian observer, GPTQConfig, gptq_quantize on the fused block kernel."""
from .api import GPTQConfig, gptq_quantize, gptq_quantize_3d  # noqa: F401
from .observer import GPTQObserverTensor  # noqa: F401

__all__ = ["GPTQConfig", "GPTQObserverTensor", "gptq_quantize", "gptq_quantize_3d"]
