"""The int8 cast of torchao/prototype/quantized_training/int8.py on the MI355X: quantize_int8_rowwise on ops.int8_train_quantize
(csrc/int8_train_kernels.hip).  Not built: Int8QuantizedTrainingLinearWeight and Int8WeightOnlyQuantizedTrainingConfig, the int8
quantized-training weight with its stochastic-rounding copy_ and its FSDP2 hooks."""
import torch
from torch import Tensor

from ao_amd import ops


@torch.no_grad()
def quantize_int8_rowwise(tensor: Tensor, stochastic_rounding: bool = False, eps: float = 1e-12):
    """Absmax int8 per row of a bf16 [R, C] tensor on the GPU -> (int8 [R, C], bf16 scale [R]): scale = amax / 127 in bf16, the codes
    rint(f32(x) * (1 / max(f32(scale), eps))) clipped to [-128, 127].  stochastic_rounding: floor(v + u) instead, u from the library's
    Philox4x32-10 stream keyed by a seed drawn from torch's generator (the reference draws u with torch.rand_like).  A transposed view is
    cast down the columns of its base, without a transposed copy; the codes come back as the same view."""
    if tensor.dim() == 2 and tensor.t().is_contiguous() and (not tensor.is_contiguous() or tensor.shape[1] % 16 != 0):
        if stochastic_rounding:
            raise NotImplementedError("quantize_int8_rowwise: stochastic rounding of a transposed view is not built (the column cast rounds to nearest)")
        q, s = ops.int8_train_quantize(tensor.t(), rows=False, cols=True, eps=eps)
        return q.t(), s
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if stochastic_rounding else None
    return ops.int8_train_quantize(tensor, rows=True, cols=False, sr_seed=seed, eps=eps)
