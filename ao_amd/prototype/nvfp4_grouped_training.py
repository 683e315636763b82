"""NVFP4 training of the MoE grouped GEMM, MI355X-native.

Host-side mirror of torchao/prototype/moe_training/nvfp4_training/nvfp4_grouped_mm.py:
  * :44-70    _to_nvfp4_rht_rs_then_scaled_grouped_mm
  * :73-337   the autograd Function _NVFP4GroupedMM (argument order and checks included)
Every token group is cast like a dense tensor under its own amaxes (the reference's grouped casts are "a launch optimization, not a
different recipe"), so the three GEMMs are nvfp4_training.py's per group, on e2m1 codes with 1 x 16 e4m3 block scales and a per-group
scale amax / 2688:
  out     [M, N]    = x_row [M, K] . W_row[e] [N, K]^T              ops.nvfp4_scaled_grouped_mm; x rowwise (RTNE), W 16 x 16 blocks
  grad_A  [M, K]    = dy_row(SR) [M, N] . W_col[e] [K, N]^T         ops.nvfp4_scaled_grouped_mm on the transposed weight cast
  grad_B  [E, N, K] = dy_col(RHT, SR) [N, M_e] . x_col(RHT) [K, M_e]^T   ops.nvfp4_grouped_mm_wgrad, contracting each group's tokens
Saved for backward: the column codes, scales and amaxes of A, the transposed weight cast, the weight amax, the offsets and the seed --
neither A nor B.  The gradient is rounded stochastically under the caller's seed and two offsets drawn on the device in every backward.
DESIGN.md 4.31.  Where the reference needs K, N and every group to be multiples of 128 (its swizzled scales), this backend keeps row-major
scales and needs multiples of 16.  Left out: the tensor-parallel / FSDP hooks, torch.compile of the Function.
"""
from typing import Optional

import torch

from .. import ops
from .mx import pad_token_groups, unpad_token_groups
from .nvfp4_training import _amax_to_scale

__all__ = ["_to_nvfp4_rht_rs_then_scaled_grouped_mm", "_NVFP4GroupedMM"]

_ALIGNMENT = 16  # the RHT's 16-row runs and the 1 x 16 blocks along the tokens must not straddle a group


def _to_nvfp4_rht_rs_then_scaled_grouped_mm(
    A: torch.Tensor,
    B: torch.Tensor,
    sign_vector,
    sr_seed: torch.Tensor,
    offs: Optional[torch.Tensor] = None,
    bias: Optional[torch.Tensor] = None,
    pad_token_groups_for_grouped_mm: bool = False,
) -> torch.Tensor:
    """Quantize and multiply grouped activations and expert weights (nvfp4_grouped_mm.py:44-70), differentiable in A and B.

    A     [M, K]      tokens, grouped by expert (cast to bfloat16 if they are not)
    B     [E, N, K]   expert weights
    offs  int32 [E]   cumulative group ends along M, read on the device
    ->    bf16 [M, N]
    The caller owns the RHT sign vector (a tuple or list of 16 values of +-1) and the stochastic-rounding seed (int64 [1] on the device).
    pad_token_groups_for_grouped_mm=True pads every group to a multiple of 16 tokens around all three GEMMs; with False every group
    end must already be a multiple of 16 (the kernels' offs contract; not checked, there is no host read).
    Refused with a ValueError that names the cause, before any launch: A not 2-D, B not 3-D, a sign vector that is not a tuple or list
    of 16 values of -1 or 1, offs missing, not 1-D int32, not contiguous or not one end an expert, sr_seed not a one-element int64
    tensor on the device, tensors that are not on the GPU or on different devices, differing contraction dimensions, K or N not
    divisible by 16, M not divisible by 16 with padding off."""
    output = _NVFP4GroupedMM.apply(A, B, sign_vector, sr_seed, offs, pad_token_groups_for_grouped_mm)
    if bias is not None:
        output = output + bias.to(output.dtype)
    return output


class _NVFP4GroupedMM(torch.autograd.Function):
    """NVFP4 grouped forward, dgrad and wgrad on the HIP casts and GEMMs (nvfp4_grouped_mm.py:73-337)."""

    @staticmethod
    def forward(ctx, input_act, weight, sign_vector, sr_seed, group_end_offsets, pad_token_groups_for_grouped_mm):
        if input_act.ndim != 2:
            raise ValueError(f"input_act must be 2D, got {input_act.ndim}D")
        if weight.ndim != 3:
            raise ValueError(f"weight must be 3D, got {weight.ndim}D")
        if not isinstance(sign_vector, (tuple, list)) or len(sign_vector) != 16:
            raise ValueError("sign_vector must be a tuple or list with 16 elements")
        if any(sign not in (-1, 1) for sign in sign_vector):
            raise ValueError("sign_vector elements must be -1 or 1")
        if group_end_offsets is None:
            raise ValueError("offs is required for NVFP4 grouped GEMM")
        if group_end_offsets.ndim != 1 or group_end_offsets.dtype != torch.int32:
            raise ValueError("offs must be a 1D int32 tensor")
        if not group_end_offsets.is_contiguous():
            raise ValueError("offs must be contiguous")
        if group_end_offsets.numel() != weight.shape[0]:
            raise ValueError("offs must contain one group-end offset per expert")
        if sr_seed.ndim != 1 or sr_seed.numel() != 1:
            raise ValueError("sr_seed must be a one-element tensor")
        if sr_seed.dtype != torch.int64:
            raise ValueError("sr_seed must be an int64 tensor")
        num_tokens, K = input_act.shape
        num_experts, N, weight_K = weight.shape
        if weight_K != K:
            raise ValueError(f"input and weight contraction dimensions differ: {K} and {weight_K}")
        if K == 0 or N == 0 or K % _ALIGNMENT != 0 or N % _ALIGNMENT != 0:
            raise ValueError(f"K and N must be divisible by {_ALIGNMENT}; got K={K}, N={N}")
        if not pad_token_groups_for_grouped_mm and num_tokens % _ALIGNMENT != 0:
            raise ValueError(f"M={num_tokens} tokens must be divisible by {_ALIGNMENT} (every token group must be 16-row aligned) when "
                             "padding is disabled; pass pad_token_groups_for_grouped_mm=True")
        # (the reference asks for the device before the shapes; here a shape is refused wherever the tensors live)
        if not (input_act.is_cuda and weight.is_cuda and group_end_offsets.is_cuda and sr_seed.is_cuda):
            raise ValueError("input_act, weight, offs and sr_seed must be GPU tensors (the MI355X backend has no CPU fallback)")
        if not (input_act.device == weight.device == group_end_offsets.device == sr_seed.device):
            raise ValueError("all tensor arguments must be on the same device")

        input_act = input_act.to(torch.bfloat16).contiguous()
        weight = weight.to(torch.bfloat16).contiguous()
        mask = ops.nvfp4_sign_mask(tuple(sign_vector))
        pad_starts = None
        if pad_token_groups_for_grouped_mm:
            # ao_moe_padded_rows(tokens, E, 16) is a multiple of 16 for every token count; the rows past the last group are capacity rows
            input_act, pad_starts, pad_ends = pad_token_groups(input_act, group_end_offsets, _ALIGNMENT)
        else:
            pad_ends = group_end_offsets
        need_col = ctx.needs_input_grad[1]  # the column cast of A only feeds the weight gradient
        x_amax = ops.nvfp4_train_group_amax(input_act, pad_ends, mask, want_rht=need_col)
        x_col_q, x_col_s, x_row_q, x_row_s = ops.nvfp4_train_quantize_row_col_grouped(input_act, x_amax, pad_ends, mask, want_col=need_col)
        w_amax = ops.nvfp4_train_weight_amax_3d(weight)
        w_q, w_s, wt_q, wt_s = ops.nvfp4_train_quantize_weight_3d(weight, w_amax)
        output = ops.nvfp4_scaled_grouped_mm(x_row_q, x_row_s, w_q, w_s, pad_ends, _amax_to_scale(x_amax[:, 1]), _amax_to_scale(w_amax))
        if pad_token_groups_for_grouped_mm:
            output = unpad_token_groups(output, group_end_offsets, pad_starts, num_tokens, _ALIGNMENT)
        ctx.save_for_backward(x_col_q, x_col_s, x_amax, wt_q, wt_s, w_amax, group_end_offsets, pad_starts, pad_ends, sr_seed)
        ctx.pad = pad_token_groups_for_grouped_mm
        ctx.num_tokens = num_tokens
        ctx.mask = mask
        return output

    @staticmethod
    def backward(ctx, grad_output):
        x_col_q, x_col_s, x_amax, wt_q, wt_s, w_amax, offs, pad_starts, pad_ends, sr_seed = ctx.saved_tensors
        grad_output = grad_output.to(torch.bfloat16).contiguous()
        if ctx.pad:
            grad_output, _, _ = pad_token_groups(grad_output, offs, _ALIGNMENT)
        need_input, need_weight = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        grad_input = grad_weight = None
        if need_input or need_weight:
            dev = grad_output.device
            dy_amax = ops.nvfp4_train_group_amax(grad_output, pad_ends, ctx.mask, want_rht=need_weight)
            # fresh offsets from the default generator of the device, drawn in nvfp4_mm_hip's order (column, then row): under graph
            # capture the generator is a side input of the graph, advanced between replays, so every backward rounds with other bits
            col_offset = torch.randint(0, 2 ** 32, (1,), dtype=torch.int64, device=dev)
            row_offset = torch.randint(0, 2 ** 32, (1,), dtype=torch.int64, device=dev)
            dy_col_q, dy_col_s, dy_row_q, dy_row_s = ops.nvfp4_train_quantize_row_col_grouped(
                grad_output, dy_amax, pad_ends, ctx.mask, sr_seed, col_offset, row_offset, want_col=need_weight, want_row=need_input)
            if need_input:
                grad_input = ops.nvfp4_scaled_grouped_mm(dy_row_q, dy_row_s, wt_q, wt_s, pad_ends, _amax_to_scale(dy_amax[:, 1]),
                                                         _amax_to_scale(w_amax))
                if ctx.pad:
                    grad_input = unpad_token_groups(grad_input, offs, pad_starts, ctx.num_tokens, _ALIGNMENT)
            if need_weight:
                grad_weight = ops.nvfp4_grouped_mm_wgrad(dy_col_q, dy_col_s, x_col_q, x_col_s, _amax_to_scale(dy_amax[:, 0]),
                                                         _amax_to_scale(x_amax[:, 0]), pad_ends)
        return grad_input, grad_weight, None, None, None, None
