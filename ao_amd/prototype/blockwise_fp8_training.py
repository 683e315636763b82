"""Blockwise float8 training of dense linears, MI355X-native: 1 x 128 activation / gradient blocks, 128 x 128 weight blocks -- the
DeepSeek-V3 recipe.

Host-side mirror of torchao/prototype/blockwise_fp8_training/linear.py:
  * :98-211   fp8_blockwise_mm, the autograd Function (argument order included)
  * :214-278  Float8BlockwiseLinear
  * :281-287  Float8BlockwiseLinearConfig and its quantize_ handler
The three GEMMs, every operand cast each call from the high-precision tensor (the reference re-casts in backward too):
  out         [M, N] = x [M, K]        x W [N, K]^T    ops.fp8_block_mm on the 1 x 128 cast of x and the 128 x 128 cast of W
  grad_input  [M, K] = grad_out [M, N] x W [N, K]      ops.fp8_block_mm on the 1 x 128 cast of grad_out and the TRANSPOSED cast of W
                                                       (codes [K, N], scales [K/128, N/128]: the same blocks, the layout of a weight [K, N])
  grad_weight [N, K] = grad_out^T      x x             ops.fp8_block_mm_wgrad on the 128 x 1 casts of grad_out and x (stored transposed)
grad_out is cast in both directions by one read of it (ops.fp8_block_train_cast(go, rows=True, cols=True)).  The casts hold RECIPROCAL
scales, which is what the GEMMs multiply by.  DESIGN.md 4.20.
The routed experts train through blockwise_fp8_grouped_training.py.
Left out: the DTensor / FSDP sharding rules of the reference's kernels, torch.compile of the Function, e5m2 / fnuz elements, fp32 operands.
"""
import torch
from torch import nn

from .. import ops
from ..quantization.config import AOBaseConfig
from ..quantization.quant_api import register_quantize_module_handler

__all__ = ["fp8_blockwise_mm", "Float8BlockwiseLinear", "Float8BlockwiseLinearConfig"]

BLOCK = 128


class fp8_blockwise_mm(torch.autograd.Function):
    """x [..., K] @ weight [N, K]^T -> [..., N] with blockwise float8 GEMMs forward and backward (linear.py:98-211).

    `use_triton` is accepted and selects nothing: there is one implementation, the HIP kernels.
    Refused with a reason, before any launch: block_size != 128; operands or out_dtype that are not bfloat16; K or N that is no multiple
    of 128 (each is a contraction dimension once and the weight's blocks are 128 x 128); a token count M that is no multiple of 128
    while the weight needs a gradient (the weight gradient's scales cover 128 tokens) -- pad the tokens or freeze the weight.  The
    forward and grad_input run for any M."""

    @classmethod
    def apply(cls, x, weight, block_size=BLOCK, out_dtype=torch.bfloat16, use_triton=False):
        # the refusals, where the grad mode of the call is still visible (inside forward it is always off)
        assert block_size == BLOCK, f"Only support block_size=128, got {block_size}"
        assert isinstance(x, torch.Tensor) and isinstance(weight, torch.Tensor), "x and weight must be tensors"
        assert x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16, (
            f"x and weight must be bfloat16 (fp32 operands are left out), got {x.dtype} and {weight.dtype}")
        assert out_dtype == torch.bfloat16, f"out_dtype must be bfloat16 (the GEMMs round their fp32 sums to bf16), got {out_dtype}"
        assert weight.ndim == 2 and x.ndim >= 1 and x.shape[-1] == weight.shape[1], (
            f"shapes {tuple(x.shape)} and {tuple(weight.shape)} are not compatible (x [..., K], weight [N, K])")
        n, k = weight.shape
        assert k > 0 and n > 0 and k % BLOCK == 0 and n % BLOCK == 0, (
            f"K and N must be positive multiples of 128 (each is a contraction dimension once), got K={k} N={n}")
        m = x.numel() // k
        needs_wgrad = torch.is_grad_enabled() and weight.requires_grad
        assert not needs_wgrad or m % BLOCK == 0, (
            f"M={m} tokens must be a multiple of 128 while the weight needs a gradient (its GEMM's scales cover 128 tokens): pad the "
            "tokens or freeze the weight")
        return super().apply(x, weight, block_size, out_dtype, use_triton)

    @staticmethod
    def forward(ctx, x, weight, block_size, out_dtype=torch.bfloat16, use_triton=False):
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(x, weight)
        x_orig_shape = x.shape
        x2 = x.reshape(-1, x_orig_shape[-1])
        (x_q, x_inv), _ = ops.fp8_block_train_cast(x2, rows=True, cols=False)
        w_q, w_inv = ops.fp8_block_train_cast_weight(weight, transposed=False)
        out = ops.fp8_block_mm(x_q, x_inv, w_q, w_inv)
        return out.reshape(*x_orig_shape[:-1], out.shape[-1])

    @staticmethod
    def backward(ctx, grad_output):
        x, weight = ctx.saved_tensors
        assert grad_output.dtype == torch.bfloat16, f"grad_output must be bfloat16, got {grad_output.dtype}"
        n, k = weight.shape
        # grad_output may be non-contiguous (a transposed or strided downstream op): the casts take contiguous rows (linear.py:148)
        go = grad_output.reshape(-1, n).contiguous()
        need_input, need_weight = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        go_rows = go_cols = None
        if need_input or need_weight:
            go_rows, go_cols = ops.fp8_block_train_cast(go, rows=need_input, cols=need_weight)
        grad_input = grad_weight = None
        if need_input:
            w_t, w_tinv = ops.fp8_block_train_cast_weight(weight, transposed=True)
            grad_input = ops.fp8_block_mm(go_rows[0], go_rows[1], w_t, w_tinv).reshape(*grad_output.shape[:-1], k)
        if need_weight:
            _, (x_t, x_tinv) = ops.fp8_block_train_cast(x.reshape(-1, k), rows=False, cols=True)
            grad_weight = ops.fp8_block_mm_wgrad(go_cols[0], go_cols[1], x_t, x_tinv)
        return grad_input, grad_weight, None, None, None


class Float8BlockwiseLinear(nn.Linear):
    """A linear layer whose three GEMMs run in blockwise float8 with dynamic casts (linear.py:214-278).  No bias: the reference's forward
    drops one silently, so constructing with bias=True raises here.  `dtype` is the GEMMs' output dtype (bfloat16)."""

    supported_dtypes = [torch.bfloat16]

    def __init__(self, *args, block_size: int = BLOCK, dtype=torch.bfloat16, use_triton=False, **kwargs):
        super().__init__(*args, **kwargs)
        assert dtype in self.supported_dtypes, f"Unsupported dtype: {dtype}. Supported dtypes: {self.supported_dtypes}"
        assert block_size == BLOCK, f"Only support block_size=128, got {block_size}"
        if self.bias is not None:
            raise ValueError("Float8BlockwiseLinear takes no bias (the reference's forward would drop it silently): construct it with "
                             "bias=False and add the bias outside")
        self.block_size = block_size
        self.dtype = dtype
        self.use_triton = use_triton

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return fp8_blockwise_mm.apply(x, self.weight, self.block_size, self.dtype, self.use_triton)

    @classmethod
    def from_float(cls, mod):
        """A Float8BlockwiseLinear that shares `mod`'s weight Parameter (linear.py:262-278)."""
        assert mod.bias is None, "unsupported: the linear has a bias"
        assert mod.in_features % BLOCK == 0, f"unsupported: in_features={mod.in_features} is no multiple of 128"
        assert mod.out_features % BLOCK == 0, f"unsupported: out_features={mod.out_features} is no multiple of 128"
        with torch.device("meta"):
            new_mod = cls(mod.in_features, mod.out_features, bias=False)
        new_mod.weight = mod.weight
        new_mod.bias = mod.bias
        return new_mod


class Float8BlockwiseLinearConfig(AOBaseConfig):
    """quantize_(model, Float8BlockwiseLinearConfig(), filter_fn=...) swaps every linear the filter passes for
    Float8BlockwiseLinear.from_float of it (linear.py:281-287)."""


@register_quantize_module_handler(Float8BlockwiseLinearConfig)
def _float8_blockwise_transform(module, config):
    return Float8BlockwiseLinear.from_float(module)
