"""MXFP8 training of dense linears and its quantize_ config, MI355X-native.

Host-side mirror of torchao/prototype/moe_training:
  * mxfp8_linear.py:27-306      _to_mxfp8_then_scaled_mm, the autograd Function mx_mm, MXFP8Linear
  * config.py:29-36, 138-252    MXFP8TrainingRecipe, MXFP8TrainingOpConfig and its quantize_ handler
  * tensor.py:34-154, 274-337   TrainingWeightWrapperBaseTensor, MXFP8TrainingWeightWrapperTensor (linear / mm / matmul / addmm and
                                _grouped_mm overrides)
  * conversion_utils.py:50-125  _swap_params
The three GEMMs of a linear (mxfp8_linear.py:85-91), every operand cast to MXFP8 along the dimension its GEMM contracts:
  out         [M, N] = x [M, K]        x W [N, K]^T    ops.mx_linear on W cast rowwise (1 x 32 along K)
  grad_input  [M, K] = grad_out [M, N] x W [N, K]      ops.mx_mm on grad_out cast rowwise and W cast colwise (32 x 1: blocks along N)
  grad_weight [N, K] = grad_out^T      x x             ops.mxfp8_mm_wgrad on the colwise casts of grad_out and x
grad_out is cast in both directions by one pass over it (mx.mxfp8_cast_both).  DESIGN.md 4.17.
Left out: the FSDP2 hooks (fsdp_pre_all_gather / fsdp_post_all_gather), the DTensor strategies and the torch version gate of
_get_tensor_cls_for_config (conversion_utils.py:32-43), MXTensor inputs, torch.compile of the Function.
"""
from dataclasses import dataclass
from enum import Enum
from typing import Any, Optional

import torch
import torch.utils._pytree as pytree
from torch import nn

from .. import ops
from ..quantization.config import AOBaseConfig, KernelPreference
from ..quantization.quant_api import register_quantize_module_handler
from .mx import BLOCK, ScaleCalculationMode, _to_mxfp8_then_scaled_grouped_mm, mxfp8_cast_both

__all__ = ["mx_mm", "_to_mxfp8_then_scaled_mm", "MXFP8Linear", "MXFP8TrainingRecipe", "MXFP8TrainingOpConfig",
           "TrainingWeightWrapperBaseTensor", "MXFP8TrainingWeightWrapperTensor", "_swap_params", "unwrap_weight"]


def _to_mxfp8_then_scaled_mm(
    input_hp: torch.Tensor,
    weight_hp: torch.Tensor,
    kernel_preference: KernelPreference,
    scale_calculation_mode: ScaleCalculationMode,
    wgrad_with_hp: bool = False,
) -> torch.Tensor:
    """input_hp [..., K] @ weight_hp [N, K]^T -> [..., N] with MXFP8 (e4m3, block 32) GEMMs forward and backward
    (mxfp8_linear.py:27-80); `wgrad_with_hp` computes grad_weight as the bf16 matmul grad_out^T @ input instead.

    kernel_preference: AUTO or EMULATED.  Both run the same HIP kernels: they compute the numerics of the reference's EMULATED path
    (operands dequantised per block, fp32 accumulation, one rounding to bf16), which on this hardware is also the fast path.
    Refused with a reason, before any launch: operands that are not bfloat16; K or N that is no multiple of 32 (each is contracted once);
    a token count M that is no multiple of 32 while the weight's gradient is computed in MXFP8 (its scales cover 32 tokens) -- pass
    wgrad_with_hp=True or freeze the weight; other kernel preferences."""
    try:
        kernel_preference = KernelPreference(kernel_preference)
    except ValueError:
        pass
    assert kernel_preference in (KernelPreference.AUTO, KernelPreference.EMULATED), (
        f"MXFP8 training on MI355X runs KernelPreference AUTO or EMULATED (the same HIP kernels), got {kernel_preference}")
    assert input_hp.dtype == torch.bfloat16 and weight_hp.dtype == torch.bfloat16, (
        f"input and weight must be bfloat16, got {input_hp.dtype} and {weight_hp.dtype}")
    assert weight_hp.ndim == 2 and input_hp.ndim >= 1 and input_hp.shape[-1] == weight_hp.shape[1], (
        f"shapes {tuple(input_hp.shape)} and {tuple(weight_hp.shape)} are not compatible (input [..., K], weight [N, K])")
    n, k = weight_hp.shape
    assert k % BLOCK == 0 and n % BLOCK == 0, f"K and N must be multiples of 32 (each is a contraction dimension once), got K={k} N={n}"
    m = input_hp.numel() // k
    needs_wgrad = torch.is_grad_enabled() and weight_hp.requires_grad
    assert wgrad_with_hp or not needs_wgrad or m % BLOCK == 0, (
        f"M={m} tokens must be a multiple of 32 (the weight gradient's scales cover 32 tokens): pass wgrad_with_hp=True or freeze the weight")
    in_elem_dtype = w_elem_dtype = grad_elem_dtype = torch.float8_e4m3fn
    # the reference's two cast-kernel choices (TRITON / CUDA) have one answer here, the HIP casts: their positions stay, unused
    return mx_mm.apply(input_hp, weight_hp, in_elem_dtype, w_elem_dtype, grad_elem_dtype, BLOCK, kernel_preference, None, None,
                       scale_calculation_mode, wgrad_with_hp)


class mx_mm(torch.autograd.Function):
    """Mirror of the reference's mx_mm (mxfp8_linear.py:83-269), its argument order included.  Call it through
    _to_mxfp8_then_scaled_mm, which checks the operands."""

    @staticmethod
    def forward(ctx, input_hp: torch.Tensor, weight_hp: torch.Tensor, in_elem_dtype: Any, w_elem_dtype: Any, grad_elem_dtype: Any,
                block_size: int, kernel_preference: KernelPreference, mxfp8_dim0_cast_kernel_choice: Any,
                mxfp8_dim1_cast_kernel_choice: Any, scale_calculation_mode: ScaleCalculationMode, wgrad_with_hp: bool):
        assert in_elem_dtype == w_elem_dtype == grad_elem_dtype == torch.float8_e4m3fn and block_size == BLOCK, (
            "mx_mm on MI355X implements float8_e4m3fn elements with block_size 32")
        ctx.save_for_backward(input_hp, weight_hp)
        ctx.scale_calculation_mode = scale_calculation_mode
        ctx.wgrad_with_hp = wgrad_with_hp
        input_orig_shape = input_hp.shape
        input_hp_r = input_hp.reshape(-1, input_orig_shape[-1])
        # input @ weight_t = output: the weight cast rowwise each call, the input inside ops.mx_linear (fused where the shape fits)
        w_q, w_s = ops.mxfp8_quantize(weight_hp.contiguous(), scale_calculation_mode)
        output = ops.mx_linear(input_hp_r, w_q, w_s, None, ops.MX_FMT_E4M3, scale_calculation_mode)
        return output.reshape(*input_orig_shape[:-1], output.shape[-1])

    @staticmethod
    def backward(ctx, grad_output_hp: torch.Tensor):
        input_hp, weight_hp = ctx.saved_tensors
        mode = ctx.scale_calculation_mode
        assert grad_output_hp.dtype == torch.bfloat16, f"grad_output must be bfloat16, got {grad_output_hp.dtype}"
        # grad_output may be non-contiguous (a transposed or strided downstream op): the casts take contiguous input (:157-162)
        grad_output_hp = grad_output_hp.contiguous()
        grad_output_orig_shape = grad_output_hp.shape
        go = grad_output_hp.reshape(-1, grad_output_orig_shape[-1])
        x = input_hp.reshape(-1, input_hp.shape[-1])
        n, k = weight_hp.shape
        need_input, need_weight = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        mx_wgrad = need_weight and not ctx.wgrad_with_hp
        if need_input and mx_wgrad:
            go_q, go_s, go_t, go_ts = mxfp8_cast_both(go, mode)
        elif need_input:
            go_q, go_s = ops.mxfp8_quantize(go, mode)
        elif mx_wgrad:
            go_t, go_ts = ops.mxfp8_quantize_colwise(go, mode)
        grad_input = grad_weight = None
        if need_input:
            # grad_output @ weight = grad_input, contracting N: the weight's 32 x 1 cast writes the codes transposed, [K][N], which is the
            # operand as ops.mx_mm stores it; its scales come as [N/32][K] and are brought to [K][N/32] by a copy of N K / 32 bytes
            w_t, w_ts = ops.mxfp8_quantize_colwise(weight_hp.contiguous(), mode)
            grad_input = ops.mx_mm(go_q, go_s, w_t.t(), w_ts.contiguous(), None, ops.MX_FMT_E4M3)
            grad_input = grad_input.reshape(*grad_output_orig_shape[:-1], k)
        if need_weight:
            if ctx.wgrad_with_hp:
                grad_weight = torch.mm(go.t(), x)
            else:
                x_t, x_ts = ops.mxfp8_quantize_colwise(x.contiguous(), mode)
                grad_weight = ops.mxfp8_mm_wgrad(go_t, go_ts, x_t, x_ts, n, k)
        return grad_input, grad_weight, None, None, None, None, None, None, None, None, None


class MXFP8Linear(nn.Linear):
    """A linear layer whose three GEMMs run in MXFP8 with dynamic casts (mxfp8_linear.py:272-306)."""

    def __init__(self, *args, kernel_preference: KernelPreference = KernelPreference.AUTO,
                 scale_calculation_mode: ScaleCalculationMode = ScaleCalculationMode.RCEIL, wgrad_with_hp: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.kernel_preference = kernel_preference
        self.scale_calculation_mode = scale_calculation_mode
        self.wgrad_with_hp = wgrad_with_hp

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        output = _to_mxfp8_then_scaled_mm(input, self.weight, kernel_preference=self.kernel_preference,
                                          scale_calculation_mode=self.scale_calculation_mode, wgrad_with_hp=self.wgrad_with_hp)
        if self.bias is not None:
            output = output + self.bias.to(output.dtype)
        return output


# ---- quantize_ -----------------------------------------------------------------------------------------------------------------------------
class MXFP8TrainingRecipe(Enum):
    """config.py:29-36"""

    MXFP8_RCEIL = "mxfp8_rceil"
    MXFP8_RCEIL_WGRAD_WITH_HP = "mxfp8_rceil_wgrad_with_hp"
    MXFP8_EMULATED_RCEIL = "mxfp8_emulated_rceil"


@dataclass
class MXFP8TrainingOpConfig(AOBaseConfig):
    """The MXFP8 training config for nn.Linear layers and grouped GEMMs (config.py:138-227).  Its quantize_ handler swaps the data of every
    parameter of the modules that pass the filter for an MXFP8TrainingWeightWrapperTensor, which sends matmuls and grouped GEMMs on the
    parameter to the MXFP8 autograd Functions and behaves like a plain tensor for every other op."""

    kernel_preference: KernelPreference = KernelPreference.AUTO  # AUTO and EMULATED run the same kernels here (_to_mxfp8_then_scaled_mm)
    out_dtype: Optional[torch.dtype] = torch.bfloat16             # of the grouped GEMMs
    wgrad_with_hp: bool = False                                   # weight gradients in bf16 instead of MXFP8
    scale_calculation_mode: ScaleCalculationMode = ScaleCalculationMode.RCEIL
    pad_token_groups_for_grouped_mm: bool = False                 # pad every token group to a multiple of 32

    @classmethod
    def from_recipe(cls, recipe: MXFP8TrainingRecipe) -> "MXFP8TrainingOpConfig":
        if recipe == MXFP8TrainingRecipe.MXFP8_RCEIL:
            return cls(kernel_preference=KernelPreference.AUTO, out_dtype=torch.bfloat16, wgrad_with_hp=False,
                       scale_calculation_mode=ScaleCalculationMode.RCEIL, pad_token_groups_for_grouped_mm=False)
        if recipe == MXFP8TrainingRecipe.MXFP8_RCEIL_WGRAD_WITH_HP:
            return cls(kernel_preference=KernelPreference.AUTO, out_dtype=torch.bfloat16, wgrad_with_hp=True,
                       scale_calculation_mode=ScaleCalculationMode.RCEIL, pad_token_groups_for_grouped_mm=False)
        if recipe == MXFP8TrainingRecipe.MXFP8_EMULATED_RCEIL:
            return cls(kernel_preference=KernelPreference.EMULATED, out_dtype=torch.bfloat16, wgrad_with_hp=False,
                       scale_calculation_mode=ScaleCalculationMode.RCEIL, pad_token_groups_for_grouped_mm=False)
        raise ValueError(f"Unsupported MXFP8 recipe: {recipe}")

    def _key(self):
        return (self.kernel_preference, self.out_dtype, self.wgrad_with_hp, self.scale_calculation_mode, self.pad_token_groups_for_grouped_mm)

    def __eq__(self, other):
        if isinstance(other, MXFP8TrainingOpConfig):
            return self._key() == other._key()
        return NotImplemented

    def __hash__(self):
        return hash(self._key())


# tensor.py:34-49 (c10d.scatter_, listed there for tensor parallelism, is added when torch.distributed provides it)
_ops_to_preserve_subclass = {
    torch.ops.aten.empty_like.default,
    torch.ops.aten.new_zeros.default,
    torch.ops.aten.slice.Tensor,
    torch.ops.aten.copy_.default,
    torch.ops.aten.view.default,
    torch.ops.aten.as_strided.default,
    torch.ops.aten._to_copy.default,  # for *.to(dtype)
    torch.ops.aten._pin_memory.default,
    torch.ops.aten.split.Tensor,
    torch.ops.aten.clone.default,
    torch.ops.aten.transpose.int,
    torch.ops.aten.t.default,
}
try:
    _ops_to_preserve_subclass.add(torch.ops.c10d.scatter_.default)
except (AttributeError, RuntimeError):  # a torch built without distributed
    pass


class _UnwrapWeight(torch.autograd.Function):
    """Unwrap the tensor subclass in a differentiable way (utils.py:496-509).  The alias it returns shares the parameter's storage and
    version counter; `_data` itself keeps no autograd history."""

    @staticmethod
    def forward(ctx, wrapper_tensor):
        return wrapper_tensor._data.detach()

    @staticmethod
    def backward(ctx, grad_output):
        return grad_output


def unwrap_weight(wrapper_tensor):
    return _UnwrapWeight.apply(wrapper_tensor)


class TrainingWeightWrapperBaseTensor(torch.Tensor):
    """A wrapper of a high-precision parameter that behaves like a plain tensor for every op but the GEMMs its subclass overrides in
    __torch_function__ (tensor.py:52-154).  A subclass names its config type in `config_cls`: that registers it for _swap_params."""

    config = None
    config_cls = None
    _by_config = {}  # config type -> wrapper class

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        if cls.config_cls is not None:
            TrainingWeightWrapperBaseTensor._by_config[cls.config_cls] = cls

    @staticmethod
    def __new__(cls, tensor: torch.Tensor, config):
        self = torch.Tensor._make_wrapper_subclass(
            cls, tensor.size(), strides=tensor.stride(), storage_offset=tensor.storage_offset(), dtype=tensor.dtype, layout=tensor.layout,
            device=tensor.device, requires_grad=tensor.requires_grad)
        self.config = config
        return self

    def __init__(self, tensor: torch.Tensor, config):
        self._data = tensor
        self.config = config

    @classmethod
    def __torch_dispatch__(cls, func, types, args, kwargs=None):
        config = None

        def unwrap(t):
            nonlocal config
            if config is None:
                config = t.config
            else:
                assert t.config == config, f"All {cls.__name__} instances must have the same config"
            return t._data

        args_unwrapped, kwargs_unwrapped = pytree.tree_map_only(cls, unwrap, (args, kwargs or {}))
        assert config is not None, f"__torch_dispatch__ called on {func} without any {cls.__name__} arguments"
        if func == torch.ops.aten.detach.default:  # detach is a special case
            return cls(args_unwrapped[0], config)
        out = func(*args_unwrapped, **kwargs_unwrapped)
        if func not in _ops_to_preserve_subclass:
            return out
        return pytree.tree_map_only(torch.Tensor, lambda x: cls(x, config), out)

    def __repr__(self):
        return f"{type(self).__name__}(data={self._data}, config={self.config})"

    def __tensor_flatten__(self):
        return ["_data"], {"config": self.config}

    @classmethod
    def __tensor_unflatten__(cls, inner_tensors, flatten_spec, outer_size, outer_stride):
        return cls(inner_tensors["_data"], flatten_spec["config"])


class MXFP8TrainingWeightWrapperTensor(TrainingWeightWrapperBaseTensor):
    """A wrapper of a high-precision parameter that overrides linear / mm / matmul / addmm and _grouped_mm to cast both operands to MXFP8
    dynamically and run the MXFP8 GEMMs, forward and backward, as its config says (tensor.py:274-337)."""

    config_cls = MXFP8TrainingOpConfig

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
            assert kwargs.get("bias", None) is None, "the MXFP8 grouped GEMM takes no bias"
            if A.ndim == 2 and B.ndim in (2, 3) and offs is not None:
                return _to_mxfp8_then_scaled_grouped_mm(
                    A, unwrap_weight(B), offs=offs, out_dtype=config.out_dtype, scale_calculation_mode=config.scale_calculation_mode,
                    wgrad_with_hp=config.wgrad_with_hp, pad_token_groups_for_grouped_mm=config.pad_token_groups_for_grouped_mm)
        elif name in ("linear", "mm", "matmul", "addmm"):
            # linear(input, W, bias) holds W [N, K]; mm / matmul(input, B) and addmm(bias, input, B) hold B = W^T [K, N]
            bias, (A, B) = (args[0], args[1:3]) if name == "addmm" else (None, args[0:2])
            assert not isinstance(A, cls), f"A should not be a {cls.__name__}"
            assert isinstance(B, cls), f"B should be a {cls.__name__}"
            config = B.config
            assert isinstance(config, MXFP8TrainingOpConfig), "expected MXFP8TrainingOpConfig"
            weight = unwrap_weight(B)
            if name == "linear":
                bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
            else:
                assert B.ndim == 2, f"{name} on a {cls.__name__} takes a 2-D weight, got {tuple(B.shape)}"
                weight = weight.t()
            result = _to_mxfp8_then_scaled_mm(A, weight, kernel_preference=config.kernel_preference,
                                              scale_calculation_mode=config.scale_calculation_mode, wgrad_with_hp=config.wgrad_with_hp)
            if bias is not None:  # (the reference's MXFP8 wrapper drops it, tensor.py:325-331; its MXFP8Linear and float8 wrapper add it)
                result = result + bias.to(result.dtype)
            return result
        # no wrapping behaviour of the super() implementation: straight to dispatch
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)


def _swap_params(module: nn.Module, *, module_filter_fn=None, config=None, target_parameter_name: Optional[str] = None) -> nn.Module:
    """Swap the data of every nn.Parameter of `module` and its children (of those that pass module_filter_fn(module, fqn), and of the
    parameter named target_parameter_name alone, when given) for the weight wrapper tensor of `config`'s type
    (MXFP8TrainingOpConfig: MXFP8TrainingWeightWrapperTensor); a wrapped parameter is left as it is, requires_grad is kept
    (conversion_utils.py:32-125)."""
    tensor_cls = TrainingWeightWrapperBaseTensor._by_config.get(type(config))
    assert tensor_cls is not None, f"Unsupported config type: {type(config)}"
    if isinstance(module, nn.Parameter) and (module_filter_fn is None or module_filter_fn(module, "")):
        if not isinstance(module.data, tensor_cls):
            return nn.Parameter(tensor_cls(module.data, config), requires_grad=module.requires_grad)
        return module

    def post_order_traversal(mod: nn.Module, cur_fqn: str = ""):
        for child_name, child in mod.named_children():
            post_order_traversal(child, child_name if cur_fqn == "" else f"{cur_fqn}.{child_name}")
        if module_filter_fn is None or module_filter_fn(mod, cur_fqn):
            for param_name, param in list(mod.named_parameters(recurse=False)):
                if target_parameter_name is not None and param_name != target_parameter_name:
                    continue
                if not isinstance(param.data, tensor_cls):
                    setattr(mod, param_name, nn.Parameter(tensor_cls(param.data, config), requires_grad=param.requires_grad))

    post_order_traversal(module)
    return module


@register_quantize_module_handler(MXFP8TrainingOpConfig)
def _moe_training_transform(module: nn.Module, config: MXFP8TrainingOpConfig, parameter_name: Optional[str] = None) -> nn.Module:
    """config.py:230-252: quantize_'s filter has chosen `module`; every parameter of it (or the named one) is wrapped."""
    return _swap_params(module, config=config, target_parameter_name=parameter_name)
