"""Blockwise float8 MoE grouped GEMM, inference forward: 1 x 128 activation blocks, 128 x 128 weight blocks, fp32 scales -- the routed
experts of the DeepSeek-V3 / R1 and Qwen3 FP8 checkpoints (`weight` e4m3 [N, K] with `weight_scale_inv` fp32 [ceil(N/128), K/128] per
expert), MI355X-native (ao_fp8_block_grouped_mm).

Upstream has this operation as a TRAINING prototype only: torchao/prototype/moe_training/blockwise_fp8/grouped_mm.py with
grouped_mm_backend.py, whose backends are DeepGEMM (NVIDIA only) and an emulation that dequantizes both operands to bf16
(blockwise_fp8_training/grouped_kernels.py:78-93).  This module is NOT a bit-level mirror of that op, and no function here carries its
name:
  * the casts are Float8Tensor's, scale = f32(bf16(amax / 448)) (float8_tensor.py:233-242, quant_primitives.py:2173-2212, :2271-2287)
    -- what the checkpoints hold and what this library's dense blockwise layers of the same model use.  The training op re-quantizes
    the weights in every forward with another arithmetic, a reciprocal scale from an fp64 division with EPS = 1e-12
    (blockwise_fp8_training/kernels.py:1031-1058); that cast is out of scope here (the DENSE linear trains with it:
    prototype/blockwise_fp8_training.py);
  * forward only: no autograd, no backward GEMMs (the mirror of the training op, with its names, its casts and all three GEMMs, is
    prototype/blockwise_fp8_grouped_training.py, DESIGN.md 4.21, which calls this module's GEMM kernel on the training casts);
  * the GEMM is the fp32 chain of the dense blockwise linear per token group (one scaled MFMA per 128-k block onto a zero accumulator,
    acc += (p * a_s) * b_s), not a bf16 dequantize followed by a bf16 grouped mm.
Float8Tensor's aten._grouped_mm keeps refusing block scales, as upstream does.
"""
from typing import Sequence

import torch

from .. import ops
from ..torch_ops import kernels

__all__ = ["Float8BlockwiseExpertWeights", "fp8_blockwise_grouped_mm"]

BLOCK = 128
_NAME = "fp8_blockwise_grouped_mm"


class Float8BlockwiseExpertWeights:
    """Expert weights in blockwise float8, what the grouped GEMM streams: data e4m3 [E, N, K] (every expert as the checkpoint stores it),
    scale fp32 [E, ceil(N/128), K/128] (the experts' weight_scale_inv, stacked).  Built directly from checkpoint tensors (any N), by one
    cast of a bf16 tensor (from_hp) or from per-expert block-scaled Float8Tensors (from_float8_tensors)."""

    def __init__(self, data: torch.Tensor, scale: torch.Tensor):
        if data.dim() != 3 or data.dtype != torch.float8_e4m3fn:
            raise ValueError(f"Float8BlockwiseExpertWeights: data must be float8_e4m3fn [E, N, K], got {data.dtype} {tuple(data.shape)}")
        e, n, k = data.shape
        if k == 0 or k % BLOCK != 0:
            raise ValueError(f"Float8BlockwiseExpertWeights: K must be a positive multiple of {BLOCK}, got {k}")
        want = (e, (n + BLOCK - 1) // BLOCK, k // BLOCK)
        if scale.dtype != torch.float32 or tuple(scale.shape) != want:
            raise ValueError(f"Float8BlockwiseExpertWeights: scale must be float32 [E, ceil(N/128), K/128] = {want}, got {scale.dtype} "
                             f"{tuple(scale.shape)}")
        self.data, self.scale = data.contiguous(), scale.contiguous()

    @classmethod
    def from_hp(cls, B_t: torch.Tensor):
        """B_t: the bf16 [E, K, N] transposed view of the [E, N, K] expert weights (what the MXFP8 entry takes), N and K multiples of
        128.  One 128 x 128 cast over the [E N, K] view: blocks never straddle experts."""
        if B_t.dim() != 3 or B_t.dtype != torch.bfloat16:
            raise ValueError(f"Float8BlockwiseExpertWeights.from_hp: B_t must be a 3-D bfloat16 tensor [E, K, N], got {B_t.dtype} {tuple(B_t.shape)}")
        e, k, n = B_t.shape
        if n % BLOCK != 0 or k % BLOCK != 0 or k == 0:
            raise ValueError(f"Float8BlockwiseExpertWeights.from_hp: N and K must be multiples of {BLOCK} (K positive), got N={n} K={k}")
        w = B_t.transpose(-2, -1).contiguous().reshape(e * n, k)
        q, s = kernels(w).fp8_quantize_block_128x128(w)
        return cls(q.reshape(e, n, k), s.reshape(e, n // BLOCK, k // BLOCK))

    @classmethod
    def from_float8_tensors(cls, tensors: Sequence):
        """Per-expert 2-D Float8Tensors with block_size [128, 128] (Float8Tensor.from_hp(w, granularity=PerBlock([128, 128])) or built from
        a checkpoint's weight / weight_scale_inv), all of one shape."""
        from ..quantization.float8_tensor import Float8Tensor

        tensors = list(tensors)
        if not tensors:
            raise ValueError("Float8BlockwiseExpertWeights.from_float8_tensors: no experts given")
        for t in tensors:
            if not isinstance(t, Float8Tensor) or t.qdata.dim() != 2 or list(t.block_size) != [BLOCK, BLOCK]:
                raise ValueError("Float8BlockwiseExpertWeights.from_float8_tensors: every expert must be a 2-D Float8Tensor with block_size "
                                 f"[128, 128], got {type(t).__name__} {getattr(t, 'block_size', None)}")
        return cls(torch.stack([t.qdata for t in tensors]), torch.stack([t.scale.to(torch.float32) for t in tensors]))

    @property
    def shape(self):  # the [E, K, N] shape of the B_t it stands for, as MXFP8ExpertWeights
        e, n, k = self.data.shape
        return torch.Size((e, k, n))


def fp8_blockwise_grouped_mm(A: torch.Tensor, experts, offs: torch.Tensor, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """A bf16 [M_total, K] (tokens grouped by expert) x experts -> bf16 [M_total, N]: the 1 x 128 cast of A over all rows, then the
    blockwise grouped GEMM -- two launches, no padding step and no host sync (offs is read on the device).
    experts: a Float8BlockwiseExpertWeights, or the bf16 [E, K, N] transposed view of the expert weights, cast on the spot (inference
    should cast once: Float8BlockwiseExpertWeights.from_hp).  offs int32 [E], cumulative group ends.  Rows past offs[-1] are zero."""
    if out_dtype != torch.bfloat16:
        raise ValueError(f"{_NAME}: only bfloat16 out_dtype is supported, got {out_dtype}")
    if A.dim() != 2 or A.dtype != torch.bfloat16:
        raise ValueError(f"{_NAME}: A must be a 2-D bfloat16 tensor [M_total, K], got {A.dtype} {tuple(A.shape)}")
    if not isinstance(experts, Float8BlockwiseExpertWeights):
        if not isinstance(experts, torch.Tensor) or experts.dim() != 3 or experts.dtype != torch.bfloat16:
            raise ValueError(f"{_NAME}: experts must be a Float8BlockwiseExpertWeights or a 3-D bfloat16 tensor [E, K, N]")
        experts = Float8BlockwiseExpertWeights.from_hp(experts)
    e, k, n = experts.shape
    if A.shape[1] != k:
        raise ValueError(f"{_NAME}: shapes {tuple(A.shape)} and {tuple(experts.shape)} are not compatible")
    if offs.dtype != torch.int32 or offs.dim() != 1 or offs.numel() != e:
        raise ValueError(f"{_NAME}: offs must be int32 [E] = [{e}], got {offs.dtype} {tuple(offs.shape)}")
    k_ = kernels(A)
    aq, a_s = k_.fp8_quantize_block_1x128(A.contiguous())
    return k_.fp8_block_grouped_mm(aq, a_s, experts.data, experts.scale, offs)
