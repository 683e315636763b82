"""NVFP4 training of dense linears and its quantize_ config, MI355X-native.

Host-side mirror of torchao/prototype/moe_training/nvfp4_training:
  * nvfp4_linear.py     the autograd Function (nvfp4_mm_triton) and nvfp4_linear
  * nvfp4_training.py   NVFP4TrainingConfig, NVFP4Linear and the quantize_ handler
  * hadamard_utils.py   DEFAULT_SIGN_VECTOR, get_wgrad_sign_vector
The three GEMMs of a linear, all on e2m1 codes with 1 x 16 e4m3 block scales and a per-tensor scale amax / 2688, all of the shape
A [M, K] . B [N, K]^T (ops.nvfp4_scaled_mm) because the column casts are written transposed:
  out         [M, N] = x_row [M, K]               . W_row [N, K]^T     x cast rowwise (RTNE), W under 16 x 16 block scales
  grad_input  [M, K] = dy_row(SR) [M, N]          . W_col [K, N]^T     the transposed cast of W from the same read and the same scales
  grad_weight [N, K] = dy_col(RHT, SR) [N, M]     . x_col(RHT, RTNE) [K, M]^T
The operands of the weight-gradient GEMM get a 16-point randomized Hadamard transform along the tokens (it cancels in the product:
the transform is orthonormal); the gradients get stochastic rounding, keyed by the module's `_sr_seed` with fresh offsets drawn on the
device in every backward.  Only the column codes and scales of x, the transposed weight cast and the amaxes are saved for backward.
The casts and their arithmetic: ops.nvfp4_train_* (csrc/quant_math.h "NVFP4 training").
Left out: the tensor-parallel protocol (nvfp4_tensor_parallel.py), the grouped (MoE) GEMM, torch.compile of the Function, fp32 operands
(cast to bf16 first, as in the reference).  Where the reference needs M, N and K to be multiples of 128 (the tile of its swizzled
scales), this backend needs only whole blocks: multiples of 16.
"""
from dataclasses import dataclass, field
from typing import Optional

import torch
from torch import nn

from .. import ops
from ..quantization.config import AOBaseConfig, KernelPreference
from ..quantization.quant_api import register_quantize_module_handler

__all__ = ["DEFAULT_SIGN_VECTOR", "get_wgrad_sign_vector", "nvfp4_linear", "nvfp4_mm_hip", "NVFP4Linear", "NVFP4TrainingConfig"]

# TransformerEngine's get_wgrad_sign_vector default, which every NVFP4 path of the reference defaults to (hadamard_utils.py)
DEFAULT_SIGN_VECTOR = (1, 1, 1, -1, 1, -1, -1, -1, -1, -1, -1, 1, -1, 1, -1, -1)
_PREFERENCES = (KernelPreference.AUTO, KernelPreference.TORCH, KernelPreference.TRITON)
_F8_F4_MAX = 2688.0  # 448 x 6: per_tensor_amax_to_scale


def get_wgrad_sign_vector(shape, device, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """A random {-1, +1} sign vector for the Hadamard transform (hadamard_utils.get_wgrad_sign_vector)."""
    return torch.where(torch.rand(shape, device=device) >= 0.5, 1, -1).to(dtype)


def _check_sign_vector(sign_vector) -> tuple:
    if isinstance(sign_vector, torch.Tensor):
        sign_vector = sign_vector.detach().cpu().reshape(-1).tolist()
    try:
        vals = tuple(int(v) for v in sign_vector)
    except TypeError:
        raise ValueError(f"the RHT sign vector must be 16 values of +1 or -1, got {sign_vector!r}") from None
    if len(vals) != 16 or any(v not in (1, -1) for v in vals):
        raise ValueError(f"the RHT sign vector must be 16 values of +1 or -1, got {len(vals)} values {vals}")
    return vals


def _check_preference(kernel_preference) -> KernelPreference:
    try:
        kernel_preference = KernelPreference(kernel_preference)
    except ValueError:
        pass
    if kernel_preference not in _PREFERENCES:
        raise ValueError("NVFP4 training on MI355X runs kernel_preference AUTO, TORCH or TRITON (one family of HIP kernels), "
                         f"got {kernel_preference!r}")
    return kernel_preference


def _refuse_tensor_parallel(process_group, world_size) -> None:
    if process_group is not None or world_size is not None:
        raise ValueError("NVFP4 training on MI355X has no tensor-parallel protocol: process_group and world_size must be None, got "
                         f"process_group={process_group!r} world_size={world_size!r}")


def _amax_to_scale(amax: torch.Tensor) -> torch.Tensor:
    return amax.to(torch.float32) / _F8_F4_MAX


class nvfp4_mm_hip(torch.autograd.Function):
    """Mirror of the reference's nvfp4_mm_triton (nvfp4_linear.py:139-314): call it through nvfp4_linear, which checks the arguments."""

    @staticmethod
    def forward(ctx, input_hp: torch.Tensor, weight_hp: torch.Tensor, bias: Optional[torch.Tensor], sr_seed: torch.Tensor, sign_vector: tuple):
        k = input_hp.shape[-1]
        n = weight_hp.shape[0]
        if input_hp.dtype != torch.bfloat16:
            input_hp = input_hp.to(torch.bfloat16)
        if weight_hp.dtype != torch.bfloat16:
            weight_hp = weight_hp.to(torch.bfloat16)
        x = input_hp.reshape(-1, k).contiguous()
        mask = ops.nvfp4_sign_mask(sign_vector)
        need_col = ctx.needs_input_grad[1]  # the column cast of x only feeds the weight gradient
        # the amaxes are launches of their own, so a caller could reduce them across ranks before the cast
        x_amax = ops.nvfp4_train_amax(x, mask, want_rht=need_col)
        x_col_q, x_col_s, x_row_q, x_row_s = ops.nvfp4_train_quantize_row_col(x, x_amax, mask, want_col=need_col)
        w = weight_hp.contiguous()
        w_amax = ops.nvfp4_train_amax(w, 0, want_rht=False)[1]
        w_q, w_s, wt_q, wt_s = ops.nvfp4_train_quantize_weight_2d(w, w_amax)
        output = ops.nvfp4_scaled_mm(x_row_q, x_row_s, w_q, w_s, _amax_to_scale(x_amax[1]), _amax_to_scale(w_amax))
        output = output.reshape(*input_hp.shape[:-1], n)
        if bias is not None:
            output = output + bias.to(output.dtype)
        ctx.save_for_backward(x_col_q, x_col_s, x_amax, wt_q, wt_s, w_amax, sr_seed)
        ctx.input_orig_shape = input_hp.shape
        ctx.has_bias = bias is not None
        ctx.mask = mask
        return output

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        x_col_q, x_col_s, x_amax, wt_q, wt_s, w_amax, sr_seed = ctx.saved_tensors
        if grad_output.dtype != torch.bfloat16:
            grad_output = grad_output.to(torch.bfloat16)
        grad_output = grad_output.contiguous()
        dy = grad_output.reshape(-1, grad_output.shape[-1])
        need_input, need_weight = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        grad_input = grad_weight = None
        if need_input or need_weight:
            dev = dy.device
            dy_amax = ops.nvfp4_train_amax(dy, ctx.mask, want_rht=need_weight)
            # fresh offsets from the default generator of the device: under graph capture it is a side input of the graph, advanced
            # between replays, so every backward rounds with other bits
            col_offset = torch.randint(0, 2 ** 32, (1,), dtype=torch.int64, device=dev)
            row_offset = torch.randint(0, 2 ** 32, (1,), dtype=torch.int64, device=dev)
            dy_col_q, dy_col_s, dy_row_q, dy_row_s = ops.nvfp4_train_quantize_row_col(
                dy, dy_amax, ctx.mask, sr_seed, col_offset, row_offset, want_col=need_weight, want_row=need_input)
            if need_input:
                grad_input = ops.nvfp4_scaled_mm(dy_row_q, dy_row_s, wt_q, wt_s, _amax_to_scale(dy_amax[1]), _amax_to_scale(w_amax))
                grad_input = grad_input.reshape(ctx.input_orig_shape)
            if need_weight:
                grad_weight = ops.nvfp4_scaled_mm(dy_col_q, dy_col_s, x_col_q, x_col_s, _amax_to_scale(dy_amax[0]), _amax_to_scale(x_amax[0]))
        grad_bias = grad_output.sum(dim=tuple(range(grad_output.dim() - 1))) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return grad_input, grad_weight, grad_bias, None, None


def nvfp4_linear(input_hp: torch.Tensor, weight_hp: torch.Tensor, bias: Optional[torch.Tensor] = None, *, sign_vector,
                 kernel_preference: KernelPreference = KernelPreference.AUTO, sr_seed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """output = input @ weight^T + bias with NVFP4 GEMMs forward and backward (nvfp4_linear.py:317-365).

    input_hp [..., K], weight_hp [N, K], bias [N] or None; operands that are not bfloat16 are cast to it first.  sign_vector: the 16
    values of +-1 of the Hadamard transform.  kernel_preference: AUTO, TORCH or TRITON, which all run the HIP kernels.  sr_seed: an int64
    tensor of one element on the device, the key of the stochastic rounding; drawn fresh if None (pass a module buffer to reproduce a run).
    Refused with a ValueError that names the cause, before any launch: another kernel preference; a sign vector that is not 16 values of
    +-1; a token count M, an N or a K that is no multiple of 16 (every one of them is contracted or cast in blocks of 16 once)."""
    _check_preference(kernel_preference)
    sign_vector = _check_sign_vector(sign_vector)
    if weight_hp.dim() != 2 or input_hp.dim() < 1 or input_hp.shape[-1] != weight_hp.shape[1]:
        raise ValueError(f"shapes {tuple(input_hp.shape)} and {tuple(weight_hp.shape)} are not compatible (input [..., K], weight [N, K])")
    n, k = weight_hp.shape
    m = input_hp.numel() // k if k else 0
    if k == 0 or m % 16 != 0 or n % 16 != 0 or k % 16 != 0:
        raise ValueError(f"NVFP4 training needs M (tokens), N and K to be multiples of 16 (whole blocks), got M={m}, N={n}, K={k}")
    if bias is not None and tuple(bias.shape) != (n,):
        raise ValueError(f"bias must have shape ({n},), got {tuple(bias.shape)}")
    if sr_seed is None:
        sr_seed = torch.randint(-(2 ** 63), 2 ** 63 - 1, (1,), dtype=torch.int64, device=input_hp.device)
    return nvfp4_mm_hip.apply(input_hp, weight_hp, bias, sr_seed, sign_vector)


def _make_rht_sign_vector(sign_vector, device) -> torch.Tensor:
    if sign_vector is None:
        if device is not None and torch.device(device).type == "meta":
            return torch.empty(16, dtype=torch.int8, device=device)
        return get_wgrad_sign_vector(16, device=device, dtype=torch.int8)
    return torch.tensor(_check_sign_vector(sign_vector), dtype=torch.int8, device=device)


@dataclass
class NVFP4TrainingConfig(AOBaseConfig):
    """quantize_(model, NVFP4TrainingConfig()) swaps every nn.Linear the filter passes for an NVFP4Linear (nvfp4_training.py:70-104).

    kernel_preference: AUTO (the default), TORCH or TRITON -- one family of HIP kernels runs whichever is named.  process_group and
    world_size: the reference's tensor-parallel fields, refused when set.  rht_sign_vector: 16 values of +-1 shared by every swapped
    module; None lets each module draw its own."""

    kernel_preference: KernelPreference = KernelPreference.AUTO
    process_group: Optional[object] = field(default=None, compare=False)
    world_size: Optional[int] = None
    rht_sign_vector: Optional[object] = field(default=None, compare=False)

    def __post_init__(self):
        self.kernel_preference = _check_preference(self.kernel_preference)
        _refuse_tensor_parallel(self.process_group, self.world_size)
        if self.rht_sign_vector is not None:
            self.rht_sign_vector = _check_sign_vector(self.rht_sign_vector)


class NVFP4Linear(nn.Linear):
    """nn.Linear whose three GEMMs run on NVFP4 codes (nvfp4_training.py:107-236).  Buffers: `_sr_seed` (int64 [1], the key of the
    stochastic rounding) and `_rht_sign_vector` (int8 [16], persistent: a checkpoint keeps the transform's basis)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, kernel_preference: KernelPreference = KernelPreference.AUTO,
                 process_group=None, world_size: Optional[int] = None, device=None, dtype=None, rht_sign_vector=None):
        _refuse_tensor_parallel(process_group, world_size)
        kernel_preference = _check_preference(kernel_preference)
        super().__init__(in_features, out_features, bias, device=device, dtype=dtype)
        self.kernel_preference = kernel_preference
        self.register_buffer("_sr_seed", torch.randint(-(2 ** 63), 2 ** 63 - 1, (1,), dtype=torch.int64, device=device))
        self.register_buffer("_rht_sign_vector", _make_rht_sign_vector(rht_sign_vector, device), persistent=True)
        self._refresh_rht_sign_vector_tuple()

    def _refresh_rht_sign_vector_tuple(self) -> None:
        v = self._rht_sign_vector
        self._rht_sign_vector_tuple = None if v.device.type == "meta" else tuple(int(s) for s in v.detach().cpu().tolist())

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._refresh_rht_sign_vector_tuple()

    @property
    def rht_sign_vector(self) -> tuple:
        if self._rht_sign_vector_tuple is None:
            self._refresh_rht_sign_vector_tuple()
        if self._rht_sign_vector_tuple is None:
            raise RuntimeError("rht_sign_vector is not materialized")
        return self._rht_sign_vector_tuple

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return nvfp4_linear(x, self.weight, self.bias, kernel_preference=self.kernel_preference, sr_seed=self._sr_seed,
                            sign_vector=self.rht_sign_vector)

    @classmethod
    def from_linear(cls, mod: nn.Linear, kernel_preference: KernelPreference = KernelPreference.AUTO, process_group=None,
                    world_size: Optional[int] = None, rht_sign_vector=None) -> "NVFP4Linear":
        if rht_sign_vector is None:
            rht_sign_vector = getattr(mod, "_rht_sign_vector", None)
        new = cls(mod.in_features, mod.out_features, mod.bias is not None, kernel_preference=kernel_preference, process_group=process_group,
                  world_size=world_size, device=mod.weight.device, dtype=mod.weight.dtype, rht_sign_vector=rht_sign_vector)
        if mod.weight.device.type != "meta":  # the module's own parameters, not copies
            new.weight = mod.weight
            if mod.bias is not None:
                new.bias = mod.bias
        return new


@register_quantize_module_handler(NVFP4TrainingConfig)
def _nvfp4_training_transform(module: nn.Module, config: NVFP4TrainingConfig, parameter_name: Optional[str] = None) -> nn.Module:
    """nvfp4_training.py:239-256: an nn.Linear becomes an NVFP4Linear on the same parameters; anything else is left as it is."""
    if isinstance(module, NVFP4Linear) or not isinstance(module, nn.Linear):
        return module
    return NVFP4Linear.from_linear(module, kernel_preference=config.kernel_preference, process_group=config.process_group,
                                   world_size=config.world_size, rht_sign_vector=config.rht_sign_vector)
