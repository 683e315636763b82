"""float8 rowwise training of the MoE grouped GEMM and its quantize_ config, MI355X-native.

Host-side mirror of torchao/prototype/moe_training:
  * fp8_grouped_mm.py:24-319   _to_fp8_rowwise_then_scaled_grouped_mm, the autograd Function _Float8GroupedMM
  * config.py:23-134           Float8TrainingRecipe, Float8TrainingOpConfig and its quantize_ handler
  * tensor.py:217-271          Float8TrainingWeightWrapperTensor (linear / mm / matmul / addmm and _grouped_mm overrides)
The three GEMMs (W is the [E, N, K] weight behind B_t), every operand cast to e4m3 with one power-of-two scale per slice along the dimension
its GEMM contracts:
  out      [M, N]    = A [M, K] x W^T          ops.fp8_grouped_mm on A cast along K and W cast along K (the [E N, K] view, rowwise)
  grad_A   [M, K]    = grad_out [M, N] x W     ops.fp8_grouped_mm on grad_out cast along N and W cast along N per expert, stored [E][K][N]
                                               (ops.fp8_train_quantize_colwise_t_3d)
  grad_W   [E, N, K] = grad_out^T x A          ops.fp8_grouped_mm_wgrad on the casts of grad_out and A along the tokens of each group
                                               (ops.fp8_train_quantize_group_colwise_t); grad_B_t is its transpose(-2, -1)
DESIGN.md 4.19.  Left out: e5m2 / fnuz operands, float32 operands and outputs, a 3-D A, the 3-D x 3-D shared-expert case, a bias,
torch.compile of the Function, the FSDP2 / DTensor hooks.
"""
from dataclasses import dataclass
from enum import Enum
from typing import Optional

import torch

from .. import ops
from ..quantization.config import AOBaseConfig
from ..quantization.quant_api import register_quantize_module_handler
from .mx import pad_token_groups, unpad_token_groups
from .mx_training import TrainingWeightWrapperBaseTensor, _moe_training_transform, unwrap_weight

__all__ = ["_to_fp8_rowwise_then_scaled_grouped_mm", "_Float8GroupedMM", "Float8TrainingRecipe", "Float8TrainingOpConfig",
           "Float8TrainingWeightWrapperTensor"]

ALIGN = 16  # tokens a group is padded to: the e4m3 MFMA's K granularity of the casts' 16-byte pieces


def _is_column_major(x: torch.Tensor) -> bool:
    """utils.py:290-303"""
    assert x.ndim == 2 or x.ndim == 3, "input tensor must be 2D or 3D"
    return x.stride(-2) == 1 and x.stride(-1) > 1


def _to_fp8_rowwise_then_scaled_grouped_mm(
    A: torch.Tensor,
    B_t: torch.Tensor,
    offs: torch.Tensor,
    out_dtype: Optional[torch.dtype] = torch.bfloat16,
    float8_dtype: torch.dtype = torch.float8_e4m3fn,
    pad_token_groups_for_grouped_mm: bool = True,
) -> torch.Tensor:
    """The reference's float8 rowwise MoE grouped GEMM (fp8_grouped_mm.py:24-62), differentiable in A and B_t (_Float8GroupedMM).

    A     bf16 [M, K]      tokens, grouped by expert, row-major
    B_t   bf16 [E, K, N]   expert weights, the transpose(-2, -1) view of [E, N, K]: strides (K N, 1, K)
    offs  int32 [E]        cumulative group ends along M
    ->    bf16 [M, N]
    Both operands of every GEMM are cast to float8_e4m3fn dynamically, one scale per row of the contraction, rounded down to a power of
    two.  pad_token_groups_for_grouped_mm=True pads every group to a multiple of 16 tokens around the GEMMs (the reference asserts the
    flag off; here the pad kernels exist).  With False the CALLER guarantees that every group size is a multiple of 16: the offsets live on
    the device and are not validated, and a group boundary inside a 16-token slab gives unspecified values in that slab's casts.
    Refused with a reason, before any launch: A not 2-D, B_t not 3-D, operands that are not bfloat16, offs not int32 [E], incompatible
    shapes, a column-major A, a B_t that is not column-major, float8_dtype other than float8_e4m3fn, out_dtype other than bfloat16, K or N
    no multiple of 128 (each is a contraction of the forward kernel once), M no multiple of 16 without padding."""
    assert A.ndim == 2, "A must be 2D"
    assert B_t.ndim == 3, "B must be 3D"
    assert float8_dtype == torch.float8_e4m3fn, (
        f"float8_dtype must be torch.float8_e4m3fn (the float8 GEMMs on MI355X multiply e4m3fn operands only), got {float8_dtype}")
    assert out_dtype == torch.bfloat16, f"Only bfloat16 out_dtype is supported, got {out_dtype}"
    assert A.dtype == torch.bfloat16, f"A must be bfloat16, got {A.dtype}"
    assert B_t.dtype == torch.bfloat16, f"B must be bfloat16, got {B_t.dtype}"
    assert offs is not None and offs.dtype == torch.int32, "offs must be an int32 tensor"
    assert A.size(-1) == B_t.size(-2), f"shape {tuple(A.shape)} and {tuple(B_t.shape)} are not compatible for _scaled_grouped_mm"
    assert offs.ndim == 1 and offs.numel() == B_t.size(0), f"offs must have one end per expert ({B_t.size(0)}), got shape {tuple(offs.shape)}"
    assert not _is_column_major(A), "A must be row-major"
    assert _is_column_major(B_t), "B must be column-major"
    k, n = B_t.shape[-2:]
    assert k % 128 == 0 and n % 128 == 0, f"K and N must be multiples of 128 (each is a contraction dimension once), got K={k} N={n}"
    assert pad_token_groups_for_grouped_mm or A.shape[0] % ALIGN == 0, (
        f"M={A.shape[0]} tokens must be a multiple of 16 (every group size must be): pass pad_token_groups_for_grouped_mm=True")
    return _Float8GroupedMM.apply(A, B_t, offs, out_dtype, float8_dtype, pad_token_groups_for_grouped_mm)


class _Float8GroupedMM(torch.autograd.Function):
    """Mirror of the reference's _Float8GroupedMM (fp8_grouped_mm.py:65-319), its argument order included: the high-precision A and B_t
    are saved and cast again in backward.  Call it through _to_fp8_rowwise_then_scaled_grouped_mm, which checks the operands."""

    @staticmethod
    def forward(ctx, A, B_t, offs, out_dtype, float8_dtype, pad_token_groups_for_grouped_mm):
        num_tokens = A.shape[0]
        if pad_token_groups_for_grouped_mm:
            A_pad, pad_starts, pad_ends = pad_token_groups(A, offs, ALIGN)
        else:
            A_pad, pad_starts, pad_ends = A.contiguous(), None, offs
        e, k, n = B_t.shape
        a_q, _, a_inv = ops.fp8_train_quantize_rowwise(A_pad, True)
        # B_t cast along K (tensor_to_scale(B_t, axiswise_dim=-2)): the rows of the contiguous [E N, K] weight behind the view
        w_q, _, w_inv = ops.fp8_train_quantize_rowwise(B_t.transpose(-2, -1).reshape(e * n, k), True)
        out = ops.fp8_grouped_mm(a_q, a_inv, w_q.view(e, n, k), w_inv.view(e, n), pad_ends)
        if pad_token_groups_for_grouped_mm:
            out = unpad_token_groups(out, offs, pad_starts, num_tokens, ALIGN)
        ctx.save_for_backward(A_pad, B_t, offs, pad_starts, pad_ends)
        ctx.pad = pad_token_groups_for_grouped_mm
        ctx.num_tokens = num_tokens
        return out

    @staticmethod
    def backward(ctx, grad_out):
        A, B_t, offs, pad_starts, pad_ends = ctx.saved_tensors
        assert grad_out.dtype == torch.bfloat16, f"grad_output must be bfloat16, got {grad_out.dtype}"
        grad_out = grad_out.contiguous()
        if ctx.pad:
            grad_out, _, _ = pad_token_groups(grad_out, offs, ALIGN)
        grad_A = grad_B_t = None
        if ctx.needs_input_grad[0]:
            # grad_A = grad_out @ W, contracting N: grad_out cast along N; W [E, N, K] cast along N per expert, stored [E][K][N]
            g_q, _, g_inv = ops.fp8_train_quantize_rowwise(grad_out, True)
            w_q_t, _, w_inv = ops.fp8_train_quantize_colwise_t_3d(B_t.transpose(-2, -1), True)
            grad_A = ops.fp8_grouped_mm(g_q, g_inv, w_q_t, w_inv, pad_ends)  # rows past offs[-1] are zero
            if ctx.pad:
                grad_A = unpad_token_groups(grad_A, offs, pad_starts, ctx.num_tokens, ALIGN)
        if ctx.needs_input_grad[1]:
            # grad_W[e] = grad_out[rows of e]^T @ A[rows of e], contracting each group's tokens
            g_t, _, g_tinv = ops.fp8_train_quantize_group_colwise_t(grad_out, pad_ends, True)
            x_t, _, x_tinv = ops.fp8_train_quantize_group_colwise_t(A, pad_ends, True)
            grad_W = ops.fp8_grouped_mm_wgrad(g_t, g_tinv, x_t, x_tinv, pad_ends, grad_out.shape[1], A.shape[1])
            grad_B_t = grad_W.transpose(-2, -1)
        return grad_A, grad_B_t, None, None, None, None


# ---- quantize_ -----------------------------------------------------------------------------------------------------------------------------
class Float8TrainingRecipe(Enum):
    """config.py:23-26"""

    FP8_ROWWISE = "fp8_rowwise"


@dataclass
class Float8TrainingOpConfig(AOBaseConfig):
    """The float8 training config for grouped GEMMs and nn.Linear layers (config.py:49-134).  Its quantize_ handler swaps the data of every
    parameter of the modules that pass the filter for a Float8TrainingWeightWrapperTensor, which sends grouped GEMMs on the parameter to
    _Float8GroupedMM, matmuls to float8.matmul_with_hp_or_float8_args, and behaves like a plain tensor for every other op."""

    float8_dtype: torch.dtype = torch.float8_e4m3fn
    out_dtype: Optional[torch.dtype] = torch.bfloat16  # of the grouped GEMMs
    pad_token_groups_for_grouped_mm: bool = False      # pad every token group to a multiple of 16
    float8_linear_recipe: str = "rowwise"              # of the linear override: "rowwise" | "rowwise_with_gw_hp" ("tensorwise" casts
                                                       # grad_output to e5m2, which float8.check_config refuses)

    def __post_init__(self):
        from ..float8 import Float8LinearConfig
        from ..float8.float8_linear import LinearMMConfig, ScaledMMConfig

        c = self._float8_linear_config = Float8LinearConfig.from_recipe_name(self.float8_linear_recipe)
        self._linear_mm_config = LinearMMConfig(
            ScaledMMConfig(c.emulate, c.gemm_config_output.use_fast_accum, False, c.pad_inner_dim),
            ScaledMMConfig(c.emulate, c.gemm_config_grad_input.use_fast_accum, False, c.pad_inner_dim),
            ScaledMMConfig(c.emulate, c.gemm_config_grad_weight.use_fast_accum, False, c.pad_inner_dim))

    @classmethod
    def from_recipe(cls, recipe: Float8TrainingRecipe) -> "Float8TrainingOpConfig":
        if recipe == Float8TrainingRecipe.FP8_ROWWISE:
            return cls()
        raise ValueError(f"Unsupported FP8 recipe: {recipe}")

    def _key(self):
        return (self.float8_dtype, self.out_dtype, self.pad_token_groups_for_grouped_mm, self.float8_linear_recipe)

    def __eq__(self, other):
        if isinstance(other, Float8TrainingOpConfig):
            return self._key() == other._key()
        return NotImplemented

    def __hash__(self):
        return hash(self._key())


class Float8TrainingWeightWrapperTensor(TrainingWeightWrapperBaseTensor):
    """A wrapper of a high-precision parameter that overrides _grouped_mm and linear / mm / matmul / addmm to cast both operands to float8
    dynamically and run the float8 GEMMs, forward and backward, as its config says (tensor.py:217-271)."""

    config_cls = Float8TrainingOpConfig

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        if name == "_grouped_mm":
            # the "2d x 3d with offsets" case of routed experts; everything else falls back to the regular grouped mm
            A, B = args[0], args[1]
            assert not isinstance(A, cls), f"A should not be a {cls.__name__}"
            assert isinstance(B, cls), f"B should be a {cls.__name__}"
            config = B.config
            offs = kwargs.get("offs", args[2] if len(args) > 2 else None)
            assert kwargs.get("bias", None) is None, "the float8 grouped GEMM takes no bias"
            if A.ndim == 2 and B.ndim in (2, 3) and offs is not None:
                return _to_fp8_rowwise_then_scaled_grouped_mm(
                    A, unwrap_weight(B), offs, out_dtype=config.out_dtype, float8_dtype=config.float8_dtype,
                    pad_token_groups_for_grouped_mm=config.pad_token_groups_for_grouped_mm)
        elif name in ("linear", "mm", "matmul", "addmm"):
            # linear(input, W, bias) holds W [N, K]; mm / matmul(input, B) and addmm(bias, input, B) hold B = W^T [K, N]
            from ..float8.float8_linear import matmul_with_hp_or_float8_args

            bias, (A, B) = (args[0], args[1:3]) if name == "addmm" else (None, args[0:2])
            assert not isinstance(A, cls), f"A should not be a {cls.__name__}"
            assert isinstance(B, cls), f"B should be a {cls.__name__}"
            config = B.config
            assert isinstance(config, Float8TrainingOpConfig), "expected Float8TrainingOpConfig"
            weight_t = unwrap_weight(B)
            if name == "linear":
                bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
                weight_t = weight_t.t()
            else:
                assert B.ndim == 2, f"{name} on a {cls.__name__} takes a 2-D weight, got {tuple(B.shape)}"
            result = matmul_with_hp_or_float8_args.apply(A, weight_t, config._linear_mm_config, config._float8_linear_config)
            if bias is not None:
                result = result + bias.to(result.dtype)
            return result
        # no wrapping behaviour of the super() implementation: straight to dispatch
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)


# config.py:230-252: quantize_'s filter has chosen the module; every parameter of it (or the named one) is wrapped
register_quantize_module_handler(Float8TrainingOpConfig)(_moe_training_transform)
