"""Low-bit optimizers (torchao/optim): Adam and AdamW with 8-bit, 4-bit or fp8 block-quantized moments, one fused HIP launch a parameter.

    from ao_amd.optim import AdamW8bit
    opt = AdamW8bit(model.parameters(), lr=1e-3)

DESIGN.md 4.26; the arithmetic contract is csrc/quant_math.h "low-bit optimizer states".
"""
from .adam import Adam4bit, Adam8bit, AdamFp8, AdamW4bit, AdamW8bit, AdamWFp8, _AdamW, step_scalars
from .subclass_4bit import OptimState4bit
from .subclass_8bit import OptimState8bit
from .subclass_fp8 import OptimStateFp8


def CPUOffloadOptimizer(*args, **kwargs):
    """torchao.optim.CPUOffloadOptimizer is not built here."""
    raise NotImplementedError("ao_amd.optim: CPUOffloadOptimizer is not supported (the moments live with their parameter on the GPU)")


__all__ = ["Adam8bit", "Adam4bit", "AdamFp8", "AdamW8bit", "AdamW4bit", "AdamWFp8", "_AdamW", "OptimState8bit", "OptimState4bit", "OptimStateFp8",
           "CPUOffloadOptimizer", "step_scalars"]
