"""Blockwise float8 training of the MoE grouped GEMM, MI355X-native: 1 x 128 activation / gradient blocks, 128 x 128 weight blocks per
expert -- the DeepSeek-V3 recipe over routed experts.

Host-side mirror of torchao/prototype/moe_training/blockwise_fp8/grouped_mm.py:
  * :31-70    _to_fp8_blockwise_then_scaled_grouped_mm
  * :73-95    _to_fp8_blockwise_then_emulated_scaled_grouped_mm
  * :98-265   the autograd Function _Float8BlockwiseGroupedMM (argument order included)
The reference runs the three GEMMs through DeepGEMM on SM90 or through an emulation that dequantizes both operands to bf16 and calls
torch._grouped_mm (grouped_mm_backend.py); here all three run on the scaled MFMA.  With W the [E, N, K] weight behind the column-major
B_t [E, K, N], every operand cast each call from the high-precision tensor (the reference re-casts in backward too):
  out     [M, N]    = A [M, K] x W^T         ops.fp8_block_grouped_mm on the 1 x 128 cast of A and the 128 x 128 cast of W (q, inv)
  grad_A  [M, K]    = grad_out [M, N] x W    ops.fp8_block_grouped_mm on the 1 x 128 cast of grad_out and the TRANSPOSED cast of W
                                             (codes [E, K, N], scales [E, K/128, N/128])
  grad_W  [E, N, K] = grad_out^T x A         ops.fp8_block_grouped_mm_wgrad on the 128 x 1 casts of grad_out and A over ALL tokens (stored
                                             transposed; their blocks sit on the global 128-token grid, whatever offs is -- what the
                                             reference's emulated wgrad feeds torch._grouped_mm); grad_B_t is its transpose(-2, -1)
grad_out is cast in both directions by one read of it.  The casts hold RECIPROCAL scales, which is what the GEMMs multiply by.
DESIGN.md 4.21.  Left out: float32 operands and outputs, e5m2 / fnuz elements, a quantize_ config (the reference has none for this op),
torch.compile of the Function, the FSDP2 / DTensor hooks.
"""
from typing import Optional

import torch

from .. import ops
from ..quantization.config import KernelPreference
from .mx import pad_token_groups, unpad_token_groups

__all__ = ["_to_fp8_blockwise_then_scaled_grouped_mm", "_to_fp8_blockwise_then_emulated_scaled_grouped_mm", "_Float8BlockwiseGroupedMM"]

BLOCK = 128
_PREFERENCES = (KernelPreference.AUTO, KernelPreference.DEEPGEMM, KernelPreference.EMULATED)


def _is_column_major(x: torch.Tensor) -> bool:
    """blockwise_fp8_training/kernels.py (_is_column_major): the last two dimensions hold the transpose of a row-major matrix"""
    return x.stride(-2) == 1 and x.stride(-1) > 1


def _to_fp8_blockwise_then_scaled_grouped_mm(
    A: torch.Tensor,
    B_t: torch.Tensor,
    offs: Optional[torch.Tensor] = None,
    out_dtype: Optional[torch.dtype] = torch.bfloat16,
    float8_dtype: torch.dtype = torch.float8_e4m3fn,
    block_size: int = BLOCK,
    pad_token_groups_for_grouped_mm: bool = True,
    kernel_preference: KernelPreference = KernelPreference.AUTO,
) -> torch.Tensor:
    """The reference's differentiable blockwise float8 grouped GEMM (grouped_mm.py:31-70), differentiable in A and B_t.

    A     bf16 [M, K]      tokens, grouped by expert, row-major
    B_t   bf16 [E, K, N]   expert weights, the transpose(-2, -1) view of [E, N, K] (per-expert column-major)
    offs  int32 [E]        cumulative group ends along M, read on the device
    ->    bf16 [M, N]
    pad_token_groups_for_grouped_mm=True pads every group to a multiple of 128 tokens around all three GEMMs, so that a 128-token block of
    the weight gradient lies in one group.  With False the group sizes are free: the forward and grad_A take any of them, and the weight
    gradient masks a block that two groups share once for each; only M itself must then be a multiple of 128 while B_t needs a gradient.
    `kernel_preference` accepts AUTO, DEEPGEMM and EMULATED and selects nothing: there is one implementation, the HIP kernels.
    Refused with a reason, before any launch: A not 2-D, B_t not 3-D, operands or out_dtype that are not bfloat16, float8_dtype other than
    float8_e4m3fn, block_size != 128, offs not int32 [E], incompatible shapes, a column-major A, a B_t that is not per-expert
    column-major, K or N no multiple of 128, M no multiple of 128 without padding while B_t needs a gradient."""
    return _Float8BlockwiseGroupedMM.apply(A, B_t, offs, out_dtype, float8_dtype, block_size, pad_token_groups_for_grouped_mm,
                                           kernel_preference)


def _to_fp8_blockwise_then_emulated_scaled_grouped_mm(
    A: torch.Tensor,
    B_t: torch.Tensor,
    offs: Optional[torch.Tensor] = None,
    out_dtype: Optional[torch.dtype] = torch.bfloat16,
    float8_dtype: torch.dtype = torch.float8_e4m3fn,
    block_size: int = BLOCK,
    pad_token_groups_for_grouped_mm: bool = True,
) -> torch.Tensor:
    """grouped_mm.py:73-95: the same op under KernelPreference.EMULATED -- which here runs the same HIP kernels."""
    return _to_fp8_blockwise_then_scaled_grouped_mm(A, B_t, offs, out_dtype, float8_dtype, block_size, pad_token_groups_for_grouped_mm,
                                                    KernelPreference.EMULATED)


class _Float8BlockwiseGroupedMM(torch.autograd.Function):
    """Mirror of the reference's _Float8BlockwiseGroupedMM (grouped_mm.py:98-265), its argument order included: the (padded)
    high-precision A and B_t are saved and cast again in backward."""

    @classmethod
    def apply(cls, A, B_t, offs=None, out_dtype=torch.bfloat16, float8_dtype=torch.float8_e4m3fn, block_size=BLOCK,
              pad_token_groups_for_grouped_mm=True, kernel_preference=KernelPreference.AUTO):
        # the refusals, where the grad mode of the call is still visible (inside forward it is always off)
        assert block_size == BLOCK, f"Only block_size=128 is supported, got {block_size}"
        assert kernel_preference in _PREFERENCES, f"kernel_preference must be AUTO, DEEPGEMM, or EMULATED, got {kernel_preference!r}"
        assert isinstance(A, torch.Tensor) and isinstance(B_t, torch.Tensor), "A and B_t must be tensors"
        assert A.ndim == 2, f"A must be 2D, got {tuple(A.shape)}"
        assert B_t.ndim == 3, f"B_t must be 3D, got {tuple(B_t.shape)}"
        assert float8_dtype == torch.float8_e4m3fn, (
            f"float8_dtype must be torch.float8_e4m3fn (the float8 GEMMs on MI355X multiply e4m3fn operands only), got {float8_dtype}")
        assert out_dtype == torch.bfloat16, f"out_dtype must be bfloat16 (the GEMMs round their fp32 sums to bf16), got {out_dtype}"
        assert A.dtype == torch.bfloat16, f"A must be bfloat16 (fp32 operands are left out), got {A.dtype}"
        assert B_t.dtype == torch.bfloat16, f"B_t must be bfloat16 (fp32 operands are left out), got {B_t.dtype}"
        e, k, n = B_t.shape
        assert isinstance(offs, torch.Tensor) and offs.dtype == torch.int32, "offs must be an int32 tensor"
        assert offs.ndim == 1 and offs.numel() == e, f"offs must have one end per expert ({e}), got shape {tuple(offs.shape)}"
        assert A.shape[-1] == k, f"shape {tuple(A.shape)} and {tuple(B_t.shape)} are not compatible"
        assert e > 0 and k > 0 and n > 0 and k % BLOCK == 0 and n % BLOCK == 0, (
            f"K and N must be positive multiples of block_size=128 (each is a contraction dimension once), got K={k} N={n}")
        assert not _is_column_major(A), "A must be row-major"
        assert _is_column_major(B_t), "B_t must be per-expert column-major"
        needs_wgrad = torch.is_grad_enabled() and B_t.requires_grad
        assert pad_token_groups_for_grouped_mm or not needs_wgrad or A.shape[0] % BLOCK == 0, (
            f"M={A.shape[0]} tokens must be a multiple of 128 while B_t needs a gradient (its GEMM's scales cover 128 tokens): pass "
            "pad_token_groups_for_grouped_mm=True or freeze B_t")
        return super().apply(A, B_t, offs, out_dtype, float8_dtype, block_size, pad_token_groups_for_grouped_mm, kernel_preference)

    @staticmethod
    def forward(ctx, A, B_t, offs, out_dtype, float8_dtype, block_size, pad_token_groups_for_grouped_mm, kernel_preference):
        num_tokens = A.shape[0]
        if pad_token_groups_for_grouped_mm:
            # ao_moe_padded_rows(tokens, E, 128) is a multiple of 128 for every token count; the rows past the last group are zero
            A_pad, pad_starts, pad_ends = pad_token_groups(A, offs, BLOCK)
        else:
            A_pad, pad_starts, pad_ends = A.contiguous(), None, offs
        (a_q, a_inv), _ = ops.fp8_block_train_cast(A_pad, rows=True, cols=False)
        w_q, w_inv = ops.fp8_block_train_cast_weight_3d(B_t.transpose(-2, -1), transposed=False)
        out = ops.fp8_block_grouped_mm(a_q, a_inv, w_q, w_inv, pad_ends)
        if pad_token_groups_for_grouped_mm:
            out = unpad_token_groups(out, offs, pad_starts, num_tokens, BLOCK)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(A_pad, B_t, offs, pad_starts, pad_ends)
        ctx.pad = pad_token_groups_for_grouped_mm
        ctx.num_tokens = num_tokens
        return out

    @staticmethod
    def backward(ctx, grad_out):
        A, B_t, offs, pad_starts, pad_ends = ctx.saved_tensors
        assert grad_out.dtype == torch.bfloat16, f"grad_output must be bfloat16, got {grad_out.dtype}"
        need_A, need_W = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        grad_out = grad_out.contiguous()
        if ctx.pad:
            grad_out, _, _ = pad_token_groups(grad_out, offs, BLOCK)
        go_rows = go_cols = None
        if need_A or need_W:
            assert not need_W or grad_out.shape[0] % BLOCK == 0, f"{grad_out.shape[0]} (padded) tokens are no multiple of 128"
            go_rows, go_cols = ops.fp8_block_train_cast(grad_out, rows=need_A, cols=need_W)
        grad_A = grad_B_t = None
        if need_A:
            # grad_A = grad_out @ W, contracting N: the same 128 x 128 blocks of W in the layout of a weight [E, K, N]
            w_t, w_tinv = ops.fp8_block_train_cast_weight_3d(B_t.transpose(-2, -1), transposed=True)
            grad_A = ops.fp8_block_grouped_mm(go_rows[0], go_rows[1], w_t, w_tinv, pad_ends)  # rows past offs[-1] are zero
            if ctx.pad:
                grad_A = unpad_token_groups(grad_A, offs, pad_starts, ctx.num_tokens, BLOCK)
        if need_W:
            # grad_W[e] = grad_out[rows of e]^T @ A[rows of e], contracting each group's tokens
            _, (x_t, x_tinv) = ops.fp8_block_train_cast(A, rows=False, cols=True)
            grad_W = ops.fp8_block_grouped_mm_wgrad(go_cols[0], go_cols[1], x_t, x_tinv, pad_ends)
            grad_B_t = grad_W.transpose(-2, -1)
        return grad_A, grad_B_t, None, None, None, None, None, None
