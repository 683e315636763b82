"""PyTorch-dispatcher registration of the MI355X kernels.

Two layers:

0. `_C_mi355_ops.so` (csrc_torch/binding.cpp): C++ TORCH_LIBRARY_IMPL registrations under the reference's own op names --
   `torchao::mxfp8_quantize`, `torchao::fused_(un)pad_token_groups`, and (with AO_MI355_OVERRIDE_ATEN=1 in the environment
   when it is loaded) `aten::_weight_int4pack_mm`, `_convert_weight_to_int4pack`, `_int_mm`, `_scaled_mm` (rowwise e4m3),
   `_scaled_grouped_mm` (MXFP8).  `load_ops_library()` loads it; importing this module does so when it has been built.
1. `ao_mi355::*` custom ops with fake (meta) kernels, so that `torch.compile` / export can trace
   through the tensor subclasses: same tensor contracts as the ATen / torchao ops they replace.
2. `install_aten_overrides()`: registers the int4 kernels as the CUDA-key (= HIP on ROCm) kernels
   of the EXISTING ATen schemas `aten::_convert_weight_to_int4pack` and `aten::_weight_int4pack_mm`
   -- the names torchao's `Int4TilePackedTo4dTensor` calls
   (quantize_/workflows/int4/int4_tile_packed_to_4d_tensor.py:202,287) -- so an unmodified torchao
   picks the MI355X kernels up through PyTorch-ROCm's dispatcher.  Opt-in (it replaces PyTorch
   core's own kernels for every caller in the process); `aten::_int_mm` is offered the same way.
"""
import os

import torch

from . import _lib, ops

__all__ = ["install_aten_overrides", "aten_overrides_installed", "kernels", "load_ops_library", "OPS_LIB_PATH"]

OPS_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_C_mi355_ops.so")


def _tracing(x) -> bool:
    """True when `x` is not a real tensor being computed on now: Dynamo / AOT / export tracing (FakeTensor, functional
    wrappers, any active dispatch mode)."""
    from torch._subclasses.fake_tensor import is_fake
    from torch.utils._python_dispatch import _get_current_dispatch_mode

    return (torch.compiler.is_compiling() or is_fake(x) or torch._is_functional_tensor(x)
            or _get_current_dispatch_mode() is not None)


def tracing(x=None) -> bool:
    """torch.compile / export / a FakeTensor in hand: only ops with fake kernels may be called."""
    return torch.compiler.is_compiling() or (x is not None and _tracing(x))


def kernels(x=None):
    """Where the subclasses' F.linear implementations get their kernels: while tracing (torch.compile / export; `x` is the
    activation) the `ao_mi355::` dispatcher ops -- they have fake kernels, so FakeTensors flow through, and inductor calls
    them as extern kernels like the reference's `extern_kernels._int_mm` (test_int8_tensor.py:276-278) -- and in eager mode
    the C-ABI wrappers directly (the dispatcher hop costs as much as a decode kernel)."""
    if torch.compiler.is_compiling() or (x is not None and _tracing(x)):
        return torch.ops.ao_mi355
    return ops

_lib_def = torch.library.Library("ao_mi355", "DEF")
_lib_def.define("weight_int4pack_mm(Tensor x, Tensor qdata, int group_size, Tensor scale_and_zero) -> Tensor")
_lib_def.define("convert_weight_to_int4pack(Tensor w_u8, int inner_k_tiles) -> Tensor")
_lib_def.define("int8_scaled_mm(Tensor xq, Tensor x_scale, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("fp8_scaled_mm(Tensor a, Tensor b, Tensor scale_a, Tensor scale_b, Tensor? bias) -> Tensor")
_lib_def.define("int8_dynamic_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("fp8_dynamic_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("int8_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("fp8_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("int8_linear_asym(Tensor x, Tensor wq, Tensor w_scale, Tensor w_row_sums, Tensor? bias) -> Tensor")
_lib_def.define("int8_linear_tensorwise(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("fp8_linear_tensorwise(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("fp8_linear_clamped(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias, float lb, float ub, bool tensorwise) -> Tensor")
_lib_def.define("int8_linear_static(Tensor x, Tensor wq, Tensor w_scale, Tensor act_scale, Tensor? act_zero_point, Tensor? w_row_sums, Tensor? bias) -> Tensor")
_lib_def.define("fp8_int4_linear(Tensor xq, Tensor x_scale, Tensor qdata, Tensor scale_and_zero, int group_size, Tensor? bias) -> Tensor")
_lib_def.define("fp8_int4_act_linear(Tensor x, Tensor qdata, Tensor scale_and_zero, int group_size, Tensor? bias) -> Tensor")
_lib_def.define("int8_quantize_rowwise(Tensor x) -> (Tensor, Tensor)")
_lib_def.define("fp8_quantize_rowwise(Tensor x) -> (Tensor, Tensor)")
_lib_def.define("mxfp8_quantize(Tensor x, str scaling_mode) -> (Tensor, Tensor)")
_lib_def.define("mxfp8_grouped_mm(Tensor a, Tensor a_scale, Tensor b, Tensor b_scale, Tensor offs) -> Tensor")
_lib_def.define("mxfp8_grouped_mm_wgrad(Tensor g_t, Tensor g_scale, Tensor x_t, Tensor x_scale, Tensor offs, int N, int K) -> Tensor")
_lib_def.define("mxfp8_mm_wgrad(Tensor g_t, Tensor g_scale, Tensor x_t, Tensor x_scale, int N, int K) -> Tensor")
_lib_def.define("mxfp8_quantize_rowcol(Tensor x, str scaling_mode) -> (Tensor, Tensor, Tensor, Tensor)")
_lib_def.define("fp8_train_quantize_group_colwise_t(Tensor x, Tensor offs, bool pow2) -> (Tensor, Tensor, Tensor)")
_lib_def.define("fp8_train_quantize_colwise_t_3d(Tensor w, bool pow2) -> (Tensor, Tensor, Tensor)")
_lib_def.define("fp8_grouped_mm_wgrad(Tensor g_t, Tensor g_inv, Tensor x_t, Tensor x_inv, Tensor? offs, int N, int K) -> Tensor")
_lib_def.define("mxfp4_quantize(Tensor x, str scaling_mode) -> (Tensor, Tensor)")
_lib_def.define("mx_mm(Tensor a, Tensor a_scale, Tensor b, Tensor b_scale, Tensor? bias, int fmt) -> Tensor")
_lib_def.define("mx_linear(Tensor x, Tensor b, Tensor b_scale, Tensor? bias, int fmt, str scaling_mode) -> Tensor")
_lib_def.define("int8_wo_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("fp8_wo_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("fp8_quantize_block_1x128(Tensor x) -> (Tensor, Tensor)")
_lib_def.define("fp8_quantize_block_128x128(Tensor w) -> (Tensor, Tensor)")
_lib_def.define("fp8_block_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("fp8_block_grouped_mm(Tensor a, Tensor a_scale, Tensor b, Tensor b_scale, Tensor offs) -> Tensor")
# (a direction that is not asked for comes back as two empty tensors: an op returns Tensors)
_lib_def.define("fp8_block_train_cast(Tensor x, bool rows, bool cols) -> (Tensor, Tensor, Tensor, Tensor)")
_lib_def.define("fp8_block_train_cast_weight(Tensor w, bool transposed) -> (Tensor, Tensor)")
_lib_def.define("fp8_block_mm_wgrad(Tensor g_t, Tensor g_inv, Tensor x_t, Tensor x_inv) -> Tensor")
_lib_def.define("fp8_block_train_cast_weight_3d(Tensor w, bool transposed) -> (Tensor, Tensor)")
_lib_def.define("fp8_block_grouped_mm_wgrad(Tensor g_t, Tensor g_inv, Tensor x_t, Tensor x_inv, Tensor? offs) -> Tensor")
_lib_def.define("nvfp4_amax_scale(Tensor x) -> Tensor")
_lib_def.define("nvfp4_quantize(Tensor x, Tensor? per_tensor_scale) -> (Tensor, Tensor)")
_lib_def.define("nvfp4_wo_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? per_tensor_scale, Tensor? bias) -> Tensor")
_lib_def.define("nvfp4_mm(Tensor a, Tensor a_scale, Tensor b, Tensor b_scale, Tensor? a_per_tensor_scale, Tensor? b_per_tensor_scale, Tensor? bias) -> Tensor")
_lib_def.define("nvfp4_linear(Tensor x, Tensor wq, Tensor w_scale, Tensor? w_per_tensor_scale, Tensor? act_per_tensor_scale, bool dynamic_per_tensor_scale, Tensor? bias) -> Tensor")
_lib_def.define("nvfp4_group_amax_scale(Tensor x, Tensor offs) -> Tensor")
_lib_def.define("nvfp4_quantize_grouped(Tensor x, Tensor? per_group_scale, Tensor offs) -> (Tensor, Tensor)")
_lib_def.define("nvfp4_grouped_mm(int kind, Tensor a, Tensor? a_scale, Tensor wq, Tensor w_scale, Tensor offs, Tensor? a_per_group_scale, Tensor? w_per_expert_scale) -> Tensor")
# same schemas as torchao::fused_pad_token_groups / fused_unpad_token_groups (kernels/mxfp8/quant.py:1244-1246, 1319-1321)
_lib_def.define("fused_pad_token_groups(Tensor inputs, Tensor offsets, int alignment_size) -> (Tensor, Tensor, Tensor)")
_lib_def.define(
    "fused_unpad_token_groups(Tensor inputs, Tensor offsets, Tensor padded_group_start_offsets, int num_tokens, int alignment_size) -> Tensor"
)

_lib_impl = torch.library.Library("ao_mi355", "IMPL", "CUDA")
_lib_impl.impl("weight_int4pack_mm", ops.weight_int4pack_mm)
_lib_impl.impl("convert_weight_to_int4pack", ops.convert_weight_to_int4pack)
_lib_impl.impl("int8_scaled_mm", ops.int8_scaled_mm)
_lib_impl.impl("fp8_scaled_mm", ops.fp8_scaled_mm)
_lib_impl.impl("int8_dynamic_linear", ops.int8_dynamic_linear)
_lib_impl.impl("fp8_dynamic_linear", ops.fp8_dynamic_linear)
_lib_impl.impl("int8_linear", ops.int8_linear)
_lib_impl.impl("fp8_linear", ops.fp8_linear)
_lib_impl.impl("int8_linear_asym", ops.int8_linear_asym)
_lib_impl.impl("int8_linear_tensorwise", ops.int8_linear_tensorwise)
_lib_impl.impl("fp8_linear_tensorwise", ops.fp8_linear_tensorwise)
_lib_impl.impl("fp8_linear_clamped", ops.fp8_linear_clamped)
_lib_impl.impl("int8_linear_static", ops.int8_linear_static)
_lib_impl.impl("fp8_int4_linear", ops.fp8_int4_linear)
_lib_impl.impl("fp8_int4_act_linear", ops.fp8_int4_act_linear)
_lib_impl.impl("int8_quantize_rowwise", ops.int8_quantize_rowwise)
_lib_impl.impl("fp8_quantize_rowwise", ops.fp8_quantize_rowwise)
_lib_impl.impl("mxfp8_quantize", lambda x, mode: ops.mxfp8_quantize(x, mode))
_lib_impl.impl("mxfp8_grouped_mm", ops.mxfp8_grouped_mm)
_lib_impl.impl("mxfp8_grouped_mm_wgrad", ops.mxfp8_grouped_mm_wgrad)
_lib_impl.impl("mxfp8_mm_wgrad", ops.mxfp8_mm_wgrad)
_lib_impl.impl("mxfp8_quantize_rowcol", lambda x, mode: ops.mxfp8_quantize_rowcol(x, mode))
_lib_impl.impl("fp8_train_quantize_group_colwise_t", ops.fp8_train_quantize_group_colwise_t)
_lib_impl.impl("fp8_train_quantize_colwise_t_3d", ops.fp8_train_quantize_colwise_t_3d)
_lib_impl.impl("fp8_grouped_mm_wgrad", ops.fp8_grouped_mm_wgrad)
_lib_impl.impl("mxfp4_quantize", lambda x, mode: ops.mxfp4_quantize(x, mode))
_lib_impl.impl("mx_mm", ops.mx_mm)
_lib_impl.impl("mx_linear", lambda x, b, b_scale, bias, fmt, mode: ops.mx_linear(x, b, b_scale, bias, fmt, mode))
_lib_impl.impl("int8_wo_linear", lambda x, wq, w_scale, bias: ops.int8_wo_linear(x, wq, w_scale, bias))
_lib_impl.impl("fp8_wo_linear", lambda x, wq, w_scale, bias: ops.fp8_wo_linear(x, wq, w_scale, bias))
_lib_impl.impl("fp8_quantize_block_1x128", ops.fp8_quantize_block_1x128)
_lib_impl.impl("fp8_quantize_block_128x128", ops.fp8_quantize_block_128x128)


def _fp8_block_train_cast(x, rows, cols):
    row, col = ops.fp8_block_train_cast(x, rows, cols)
    none = lambda: (x.new_empty((0,), dtype=torch.float8_e4m3fn), x.new_empty((0,), dtype=torch.float32))  # noqa: E731
    return (*(row or none()), *(col or none()))


_lib_impl.impl("fp8_block_train_cast", _fp8_block_train_cast)
_lib_impl.impl("fp8_block_train_cast_weight", lambda w, transposed: ops.fp8_block_train_cast_weight(w, bool(transposed)))
_lib_impl.impl("fp8_block_mm_wgrad", ops.fp8_block_mm_wgrad)
_lib_impl.impl("fp8_block_train_cast_weight_3d", lambda w, transposed: ops.fp8_block_train_cast_weight_3d(w, bool(transposed)))
_lib_impl.impl("fp8_block_grouped_mm_wgrad", ops.fp8_block_grouped_mm_wgrad)
_lib_impl.impl("fp8_block_linear", lambda x, wq, w_scale, bias: ops.fp8_block_linear(x, wq, w_scale, bias))
_lib_impl.impl("fp8_block_grouped_mm", lambda a, a_scale, b, b_scale, offs: ops.fp8_block_grouped_mm(a, a_scale, b, b_scale, offs))
_lib_impl.impl("nvfp4_amax_scale", ops.nvfp4_amax_scale)
_lib_impl.impl("nvfp4_quantize", ops.nvfp4_quantize)
_lib_impl.impl("nvfp4_wo_linear", lambda x, wq, w_scale, p, bias: ops.nvfp4_wo_linear(x, wq, w_scale, p, bias))
_lib_impl.impl("nvfp4_mm", lambda a, a_scale, b, b_scale, pa, pb, bias: ops.nvfp4_mm(a, a_scale, b, b_scale, pa, pb, bias))
_lib_impl.impl("nvfp4_linear", ops.nvfp4_linear)
_lib_impl.impl("nvfp4_group_amax_scale", ops.nvfp4_group_amax_scale)
_lib_impl.impl("nvfp4_quantize_grouped", ops.nvfp4_quantize_grouped)
_lib_impl.impl("nvfp4_grouped_mm", lambda kind, a, a_scale, wq, w_scale, offs, pa, pb: ops.nvfp4_grouped_mm(kind, a, a_scale, wq, w_scale, offs, pa, pb))
_lib_impl.impl("fused_pad_token_groups", ops.fused_pad_token_groups)
_lib_impl.impl("fused_unpad_token_groups", ops.fused_unpad_token_groups)


@torch.library.register_fake("ao_mi355::weight_int4pack_mm")
def _(x, qdata, group_size, scale_and_zero):
    return x.new_empty((x.shape[0], qdata.shape[0] * 8), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::convert_weight_to_int4pack")
def _(w_u8, inner_k_tiles):
    n, kh = w_u8.shape
    return w_u8.new_empty((n // 8, (kh * 2) // (inner_k_tiles * 16), 32, inner_k_tiles // 2), dtype=torch.int32)


@torch.library.register_fake("ao_mi355::int8_scaled_mm")
def _(xq, x_scale, wq, w_scale, bias):
    return xq.new_empty((xq.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_scaled_mm")
def _(a, b, scale_a, scale_b, bias):
    return a.new_empty((a.shape[0], b.shape[1]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::int8_dynamic_linear")
def _(x, wq, w_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_dynamic_linear")
def _(x, wq, w_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::int8_linear")
def _(x, wq, w_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_linear")
def _(x, wq, w_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::int8_linear_asym")
def _(x, wq, w_scale, w_row_sums, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::int8_linear_tensorwise")
def _(x, wq, w_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_linear_tensorwise")
def _(x, wq, w_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_linear_clamped")
def _(x, wq, w_scale, bias, lb, ub, tensorwise):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::int8_linear_static")
def _(x, wq, w_scale, act_scale, act_zero_point, w_row_sums, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_int4_linear")
def _(xq, x_scale, qdata, scale_and_zero, group_size, bias):
    return xq.new_empty((xq.shape[0], qdata.shape[0] * 8), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_int4_act_linear")
def _(x, qdata, scale_and_zero, group_size, bias):
    return x.new_empty((x.shape[0], qdata.shape[0] * 8), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::int8_quantize_rowwise")
def _(x):
    return x.new_empty(x.shape, dtype=torch.int8), x.new_empty((x.shape[0], 1), dtype=torch.float32)


@torch.library.register_fake("ao_mi355::fp8_quantize_rowwise")
def _(x):
    return x.new_empty(x.shape, dtype=torch.float8_e4m3fn), x.new_empty((x.shape[0], 1), dtype=torch.float32)


@torch.library.register_fake("ao_mi355::mxfp8_quantize")
def _(x, scaling_mode):
    return (x.new_empty(x.shape, dtype=torch.float8_e4m3fn),
            x.new_empty((*x.shape[:-1], x.shape[-1] // 32), dtype=torch.float8_e8m0fnu))


@torch.library.register_fake("ao_mi355::mxfp8_grouped_mm")
def _(a, a_scale, b, b_scale, offs):
    return a.new_empty((a.shape[0], b.shape[1]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::mxfp8_grouped_mm_wgrad")
def _(g_t, g_scale, x_t, x_scale, offs, N, K):
    return g_t.new_empty((offs.shape[0], N, K), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::mxfp8_mm_wgrad")
def _(g_t, g_scale, x_t, x_scale, N, K):
    return g_t.new_empty((N, K), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_train_quantize_group_colwise_t")
def _(x, offs, pow2):
    r, c = x.shape
    e = offs.shape[0]
    return (x.new_empty((c, r), dtype=torch.float8_e4m3fn), x.new_empty((e, c), dtype=torch.float32), x.new_empty((e, c), dtype=torch.float32))


@torch.library.register_fake("ao_mi355::fp8_train_quantize_colwise_t_3d")
def _(w, pow2):
    e, r, c = w.shape
    return (w.new_empty((e, c, r), dtype=torch.float8_e4m3fn), w.new_empty((e, c), dtype=torch.float32), w.new_empty((e, c), dtype=torch.float32))


@torch.library.register_fake("ao_mi355::fp8_grouped_mm_wgrad")
def _(g_t, g_inv, x_t, x_inv, offs, N, K):
    return g_t.new_empty((1 if offs is None else offs.shape[0], N, K), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_block_train_cast")
def _(x, rows, cols):
    r, c = x.shape
    e = lambda on, shape, dt: x.new_empty(shape if on else (0,), dtype=dt)  # noqa: E731
    return (e(rows, (r, c), torch.float8_e4m3fn), e(rows, (r, c // 128), torch.float32),
            e(cols, (c, r), torch.float8_e4m3fn), e(cols, (r // 128, c), torch.float32))


@torch.library.register_fake("ao_mi355::fp8_block_train_cast_weight")
def _(w, transposed):
    n, k = (w.shape[1], w.shape[0]) if transposed else w.shape
    return w.new_empty((n, k), dtype=torch.float8_e4m3fn), w.new_empty((n // 128, k // 128), dtype=torch.float32)


@torch.library.register_fake("ao_mi355::fp8_block_mm_wgrad")
def _(g_t, g_inv, x_t, x_inv):
    return g_t.new_empty((g_t.shape[0], x_t.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_block_train_cast_weight_3d")
def _(w, transposed):
    e, n, k = (w.shape[0], w.shape[2], w.shape[1]) if transposed else w.shape
    return w.new_empty((e, n, k), dtype=torch.float8_e4m3fn), w.new_empty((e, n // 128, k // 128), dtype=torch.float32)


@torch.library.register_fake("ao_mi355::fp8_block_grouped_mm_wgrad")
def _(g_t, g_inv, x_t, x_inv, offs):
    return g_t.new_empty((1 if offs is None else offs.shape[0], g_t.shape[0], x_t.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::mxfp8_quantize_rowcol")
def _(x, scaling_mode):
    r, c = x.shape
    return (x.new_empty((r, c), dtype=torch.float8_e4m3fn), x.new_empty((r, c // 32), dtype=torch.float8_e8m0fnu),
            x.new_empty((c, r), dtype=torch.float8_e4m3fn).t(), x.new_empty((r // 32, c), dtype=torch.float8_e8m0fnu).t())


@torch.library.register_fake("ao_mi355::mxfp4_quantize")
def _(x, scaling_mode):
    return (x.new_empty((*x.shape[:-1], x.shape[-1] // 2), dtype=torch.uint8),
            x.new_empty((*x.shape[:-1], x.shape[-1] // 32), dtype=torch.float8_e8m0fnu))


@torch.library.register_fake("ao_mi355::mx_mm")
def _(a, a_scale, b, b_scale, bias, fmt):
    return a.new_empty((a.shape[0], b.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::mx_linear")
def _(x, b, b_scale, bias, fmt, scaling_mode):
    return x.new_empty((x.shape[0], b.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::int8_wo_linear")
def _(x, wq, w_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_wo_linear")
def _(x, wq, w_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_quantize_block_1x128")
def _(x):
    return x.new_empty(x.shape, dtype=torch.float8_e4m3fn), x.new_empty((*x.shape[:-1], x.shape[-1] // 128), dtype=torch.float32)


@torch.library.register_fake("ao_mi355::fp8_quantize_block_128x128")
def _(w):
    return w.new_empty(w.shape, dtype=torch.float8_e4m3fn), w.new_empty((w.shape[0] // 128, w.shape[1] // 128), dtype=torch.float32)


@torch.library.register_fake("ao_mi355::fp8_block_linear")
def _(x, wq, w_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fp8_block_grouped_mm")
def _(a, a_scale, b, b_scale, offs):
    return a.new_empty((a.shape[0], b.shape[1]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::nvfp4_amax_scale")
def _(x):
    return x.new_empty((), dtype=torch.float32)


@torch.library.register_fake("ao_mi355::nvfp4_quantize")
def _(x, per_tensor_scale):
    return (x.new_empty((*x.shape[:-1], x.shape[-1] // 2), dtype=torch.uint8),
            x.new_empty((*x.shape[:-1], x.shape[-1] // 16), dtype=torch.float8_e4m3fn))


@torch.library.register_fake("ao_mi355::nvfp4_wo_linear")
def _(x, wq, w_scale, per_tensor_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::nvfp4_mm")
def _(a, a_scale, b, b_scale, a_per_tensor_scale, b_per_tensor_scale, bias):
    return a.new_empty((a.shape[0], b.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::nvfp4_linear")
def _(x, wq, w_scale, w_per_tensor_scale, act_per_tensor_scale, dynamic_per_tensor_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::nvfp4_group_amax_scale")
def _(x, offs):
    return x.new_empty((offs.shape[0],), dtype=torch.float32)


@torch.library.register_fake("ao_mi355::nvfp4_quantize_grouped")
def _(x, per_group_scale, offs):
    return (x.new_empty((x.shape[0], x.shape[1] // 2), dtype=torch.uint8),
            x.new_empty((x.shape[0], x.shape[1] // 16), dtype=torch.float8_e4m3fn))


@torch.library.register_fake("ao_mi355::nvfp4_grouped_mm")
def _(kind, a, a_scale, wq, w_scale, offs, a_per_group_scale, w_per_expert_scale):
    return a.new_empty((a.shape[0], wq.shape[1]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::fused_pad_token_groups")
def _(inputs, offsets, alignment_size):
    rows = inputs.shape[0] + offsets.shape[0] * alignment_size
    rows = (rows + alignment_size - 1) // alignment_size * alignment_size
    return (inputs.new_empty((rows, inputs.shape[1])), offsets.new_empty(offsets.shape), offsets.new_empty(offsets.shape))


@torch.library.register_fake("ao_mi355::fused_unpad_token_groups")
def _(inputs, offsets, padded_group_start_offsets, num_tokens, alignment_size):
    return inputs.new_empty((num_tokens, inputs.shape[1]))


# ---- autograd: these are inference kernels ------------------------------------------------------------------------------------
# Without an Autograd-key registration PyTorch warns on every call that sees a tensor requiring grad ("an autograd kernel was not
# registered": 34 warnings in the round-2 GPU log).  The ops get an explicit FALLTHROUGH on the Autograd key: forward works on any
# input, the outputs are cut off from the graph -- what the reference's inference subclasses do too (their aten kernels run on
# `requires_grad=False` parameters).  (A backward stub that raises was tried first: AOT autograd traces the joint graph of a
# module whose bias requires grad and would hit it at torch.compile time.)
_lib_autograd = torch.library.Library("ao_mi355", "IMPL", "Autograd")
for _name in ("weight_int4pack_mm", "convert_weight_to_int4pack", "int8_scaled_mm", "fp8_scaled_mm", "int8_dynamic_linear", "fp8_dynamic_linear",
              "int8_linear", "fp8_linear", "int8_linear_asym", "int8_linear_tensorwise", "fp8_linear_tensorwise", "fp8_linear_clamped",
              "int8_linear_static", "fp8_int4_linear", "fp8_int4_act_linear", "int8_quantize_rowwise", "fp8_quantize_rowwise", "mxfp8_quantize", "mxfp8_grouped_mm",
              "mxfp8_grouped_mm_wgrad", "mxfp8_mm_wgrad", "mxfp8_quantize_rowcol",
              "fp8_train_quantize_group_colwise_t", "fp8_train_quantize_colwise_t_3d", "fp8_grouped_mm_wgrad",
              "fused_pad_token_groups", "fused_unpad_token_groups", "mxfp4_quantize", "mx_mm", "mx_linear", "int8_wo_linear", "fp8_wo_linear",
              "fp8_quantize_block_1x128", "fp8_quantize_block_128x128", "fp8_block_linear", "fp8_block_grouped_mm",
              "fp8_block_train_cast", "fp8_block_train_cast_weight", "fp8_block_mm_wgrad",
              "fp8_block_train_cast_weight_3d", "fp8_block_grouped_mm_wgrad",
              "nvfp4_amax_scale", "nvfp4_quantize", "nvfp4_wo_linear", "nvfp4_mm", "nvfp4_linear",
              "nvfp4_group_amax_scale", "nvfp4_quantize_grouped", "nvfp4_grouped_mm"):
    _lib_autograd.impl(_name, torch.library.fallthrough_kernel)


# ---- the C++ registrations (ao_amd/csrc_torch/binding.cpp -> _C_mi355_ops.so) ------------------------------------------
# torchao::mxfp8_quantize / fused_pad_token_groups / fused_unpad_token_groups / mx_block_rearrange_2d_M_groups are IMPLEMENTED in the .so under the
# reference's names (TORCH_LIBRARY_IMPL(torchao, CUDA)); their schemas are defined by torchao's Python when it is imported
# (prototype/mx_formats/kernels.py:1022-1026, moe_training/kernels/mxfp8/quant.py:1244-1246, 1319-1321) and by this module
# otherwise.  Dropped into a torchao checkout as torchao/_C_mi355_ops.so the library is found by torchao's own loader
# (torchao/__init__.py:89-94).
_TORCHAO_SCHEMAS = {
    "mxfp8_quantize": "mxfp8_quantize(Tensor input, bool rowwise, bool colwise, int scale_dim_x, int scale_dim_y, str fp8_format, "
                      "str scaling_mode) -> (Tensor, Tensor, Tensor, Tensor)",
    "fused_pad_token_groups": "fused_pad_token_groups(Tensor inputs, Tensor group_offsets, int alignment_size) -> (Tensor, Tensor, Tensor)",
    "fused_unpad_token_groups": "fused_unpad_token_groups(Tensor inputs, Tensor group_offsets, Tensor padded_group_start_offsets, "
                                "int num_tokens, int alignment_size) -> Tensor",
    # (kernels/mxfp8/quant.py:969-973)
    "mx_block_rearrange_2d_M_groups": "mx_block_rearrange_2d_M_groups(Tensor scales_tensor, Tensor input_offsets, int chunks_per_tb) -> Tensor",
}
_ops_lib_loaded = False
_torchao_def = None


def load_ops_library() -> bool:
    """torch.ops.load_library(_C_mi355_ops.so) once; defines the torchao:: schemas if nobody has.  Returns False when the
    library has not been built (python -m ao_amd.build)."""
    global _ops_lib_loaded, _torchao_def
    if _ops_lib_loaded:
        return True
    if not os.path.exists(OPS_LIB_PATH):
        return False
    _lib.lib()  # the C-ABI library the ops library links against (same directory; loaded first so that it resolves)
    torch.ops.load_library(OPS_LIB_PATH)
    _torchao_def = torch.library.Library("torchao", "FRAGMENT")
    for name, schema in _TORCHAO_SCHEMAS.items():
        if not _schema_defined(f"torchao::{name}"):
            _torchao_def.define(schema)
    _register_torchao_fakes()
    _ops_lib_loaded = True
    return True


def _schema_defined(qualname: str) -> bool:
    try:
        torch._C._dispatch_find_schema_or_throw(qualname, "")
        return True
    except RuntimeError:
        return False


def _register_torchao_fakes():
    def _try(name, fn):
        try:
            torch.library.register_fake(f"torchao::{name}")(fn)
        except RuntimeError:
            pass  # torchao's own Python registered one already

    def mx_fake(input, rowwise, colwise, scale_dim_x, scale_dim_y, fp8_format, scaling_mode):
        r, c = input.shape
        e = lambda *shape, dt: input.new_empty(shape, dtype=dt)  # noqa: E731
        out_r = e(r, c, dt=torch.float8_e4m3fn) if rowwise else e(0, dt=torch.float8_e4m3fn)
        sc_r = e(r, c // 32, dt=torch.float8_e8m0fnu) if rowwise else e(0, dt=torch.float8_e8m0fnu)
        out_c = e(c, r, dt=torch.float8_e4m3fn).t() if colwise else e(0, dt=torch.float8_e4m3fn)
        sc_c = e(r // 32, c, dt=torch.float8_e8m0fnu).t() if colwise else e(0, dt=torch.float8_e8m0fnu)
        return out_r, out_c, sc_r, sc_c

    def pad_fake(inputs, group_offsets, alignment_size):
        rows = inputs.shape[0] + group_offsets.shape[0] * alignment_size
        rows = (rows + alignment_size - 1) // alignment_size * alignment_size
        return (inputs.new_empty((rows, inputs.shape[1])), group_offsets.new_empty(group_offsets.shape), group_offsets.new_empty(group_offsets.shape))

    def unpad_fake(inputs, group_offsets, padded_group_start_offsets, num_tokens, alignment_size):
        return inputs.new_empty((num_tokens, inputs.shape[1]))

    def rearrange_fake(scales_tensor, input_offsets, chunks_per_tb):  # (kernels/mxfp8/quant.py:1228-1247)
        rows, cols = scales_tensor.shape
        return scales_tensor.new_empty((rows + input_offsets.shape[0] * 128, (cols + 3) // 4 * 4))

    _try("mx_block_rearrange_2d_M_groups", rearrange_fake)
    _try("mxfp8_quantize", mx_fake)
    _try("fused_pad_token_groups", pad_fake)
    _try("fused_unpad_token_groups", unpad_fake)


_aten_impl = None


def aten_overrides_installed() -> bool:
    if _aten_impl is not None:
        return True
    return bool(_ops_lib_loaded and torch.ops.ao_mi355_c.aten_overrides_active())


def install_aten_overrides(int_mm: bool = False) -> None:
    """Make `torch.ops.aten._weight_int4pack_mm` / `_convert_weight_to_int4pack` (and optionally
    `_int_mm`) run the MI355X kernels for GPU tensors.  Idempotent."""
    global _aten_impl
    if _aten_impl is not None:
        return
    import warnings

    lib = torch.library.Library("aten", "IMPL")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "Overriding a previously registered kernel": that is the point
        lib.impl("_weight_int4pack_mm", lambda x, q, g, sz: ops.weight_int4pack_mm(x, q, g, sz), "CUDA")
        lib.impl("_convert_weight_to_int4pack", lambda w, ikt: ops.convert_weight_to_int4pack(w, ikt), "CUDA")
        if int_mm:
            lib.impl("_int_mm", lambda a, b: ops.int_mm(a, b), "CUDA")
    _aten_impl = lib


# ---- NF4 (QLoRA) weights (ops.py "NF4"): definitions, CUDA kernels, fakes, autograd fallthrough -----------------------------
# (the gradient of linear_nf4 lives in LinearNF4, ao_amd/quantization/nf4_tensor.py: these ops are its forward pieces)
_lib_def.define("nf4_block_absmax(Tensor x, int block_size) -> Tensor")
_lib_def.define("nf4_quantize(Tensor x, Tensor absmax, Tensor mean, int block_size, int scaler_block_size) -> (Tensor, Tensor, Tensor)")
_lib_def.define("nf4_dequantize(Tensor codes, Tensor scalers, Tensor factors, Tensor mean, int block_size, int scaler_block_size) -> Tensor")
_lib_def.define("nf4_linear(Tensor x, Tensor codes, Tensor scalers, Tensor factors, Tensor mean, int n, int k, int block_size, "
                "int scaler_block_size) -> Tensor")
_lib_impl.impl("nf4_block_absmax", ops.nf4_block_absmax)
_lib_impl.impl("nf4_quantize", ops.nf4_quantize)
_lib_impl.impl("nf4_dequantize", ops.nf4_dequantize)
_lib_impl.impl("nf4_linear", lambda x, codes, scalers, factors, mean, n, k, block_size, scaler_block_size: ops.nf4_linear(
    x, codes, scalers, factors, mean, n, k, block_size, scaler_block_size))


@torch.library.register_fake("ao_mi355::nf4_block_absmax")
def _(x, block_size):
    return x.new_empty((x.numel() // block_size,), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::nf4_quantize")
def _(x, absmax, mean, block_size, scaler_block_size):
    n = x.numel()
    return (x.new_empty((n // 2,), dtype=torch.uint8), x.new_empty((n // block_size,), dtype=torch.int8),
            x.new_empty((n // (block_size * scaler_block_size),), dtype=torch.bfloat16))


@torch.library.register_fake("ao_mi355::nf4_dequantize")
def _(codes, scalers, factors, mean, block_size, scaler_block_size):
    return codes.new_empty((codes.numel() * 2,), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::nf4_linear")
def _(x, codes, scalers, factors, mean, n, k, block_size, scaler_block_size):
    return x.new_empty((x.shape[0], n), dtype=torch.bfloat16)


for _name in ("nf4_block_absmax", "nf4_quantize", "nf4_dequantize", "nf4_linear"):
    _lib_autograd.impl(_name, torch.library.fallthrough_kernel)


# ---- low-bit optimizers (ops.py "low-bit optimizers"): the two casts and the in-place step ----------------------------------
# (the (x!) annotations are the schema form of mutates_args: p and every moment's codes and scale are written in place)
_lib_def.define("optim_quantize(Tensor src, int format, int block_size, Tensor? qmap) -> (Tensor, Tensor)")
_lib_def.define("optim_dequantize(Tensor codes, Tensor scale, int format, int block_size, Tensor? qmap, ScalarType dtype) -> Tensor")
_lib_def.define("optim_adam_step(Tensor(a!) p, Tensor grad, Tensor(b!) m_codes, Tensor(c!)? m_scale, Tensor? m_qmap, Tensor(d!) v_codes, "
                "Tensor(e!)? v_scale, Tensor? v_qmap, Tensor(f!)? vmax_codes, Tensor(g!)? vmax_scale, Tensor? vmax_qmap, int format, int block_size, "
                "float[] scalars, bool is_adamw, bool sr, int seed, int step, int param_index, int max_workgroups) -> ()")
_lib_impl.impl("optim_quantize", lambda src, format, block_size, qmap: ops.optim_quantize(src, format, block_size, qmap))
_lib_impl.impl("optim_dequantize", lambda codes, scale, format, block_size, qmap, dtype: ops.optim_dequantize(codes, scale, format, block_size, qmap, dtype))
_lib_impl.impl("optim_adam_step", ops.optim_adam_step)


@torch.library.register_fake("ao_mi355::optim_quantize")
def _(src, format, block_size, qmap):
    n = src.numel()
    if format in (2, 3):
        codes = src.new_empty((n // 2,), dtype=torch.uint8)
    else:
        codes = src.new_empty(src.shape, dtype=torch.float8_e4m3fn if format == 4 else torch.uint8)
    return codes, src.new_empty((n // block_size,), dtype=torch.float32)


@torch.library.register_fake("ao_mi355::optim_dequantize")
def _(codes, scale, format, block_size, qmap, dtype):
    return codes.new_empty((codes.numel() * (2 if format in (2, 3) else 1),), dtype=dtype)


@torch.library.register_fake("ao_mi355::optim_adam_step")
def _(p, grad, m_codes, m_scale, m_qmap, v_codes, v_scale, v_qmap, vmax_codes, vmax_scale, vmax_qmap, format, block_size, scalars, is_adamw, sr,
      seed, step, param_index, max_workgroups):
    return None


for _name in ("optim_quantize", "optim_dequantize", "optim_adam_step"):
    _lib_autograd.impl(_name, torch.library.fallthrough_kernel)


# ---- SmoothQuant (ops.py "SmoothQuant"): the int8 linears with the activation pre-scale folded into the cast -----------------
# (the twins of int8_linear / int8_linear_tensorwise / int8_linear_static, with `pre` bf16 [K] after the activation)
_lib_def.define("int8_linear_prescaled(Tensor x, Tensor pre, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("int8_linear_tensorwise_prescaled(Tensor x, Tensor pre, Tensor wq, Tensor w_scale, Tensor? bias) -> Tensor")
_lib_def.define("int8_linear_static_prescaled(Tensor x, Tensor pre, Tensor wq, Tensor w_scale, Tensor act_scale, Tensor? act_zero_point, "
                "Tensor? w_row_sums, Tensor? bias) -> Tensor")
_lib_impl.impl("int8_linear_prescaled", ops.int8_linear_prescaled)
_lib_impl.impl("int8_linear_tensorwise_prescaled", ops.int8_linear_tensorwise_prescaled)
_lib_impl.impl("int8_linear_static_prescaled", ops.int8_linear_static_prescaled)


@torch.library.register_fake("ao_mi355::int8_linear_prescaled")
def _(x, pre, wq, w_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::int8_linear_tensorwise_prescaled")
def _(x, pre, wq, w_scale, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


@torch.library.register_fake("ao_mi355::int8_linear_static_prescaled")
def _(x, pre, wq, w_scale, act_scale, act_zero_point, w_row_sums, bias):
    return x.new_empty((x.shape[0], wq.shape[0]), dtype=torch.bfloat16)


for _name in ("int8_linear_prescaled", "int8_linear_tensorwise_prescaled", "int8_linear_static_prescaled"):
    _lib_autograd.impl(_name, torch.library.fallthrough_kernel)


load_ops_library()
