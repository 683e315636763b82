"""Int8 mixed-precision training (mirrors torchao/prototype/quantized_training/int8_mixed_precision.py) on the MI355X.

`quantize_(model, Int8MixedPrecisionTrainingConfig())` keeps each linear's weight in bf16 and runs the GEMMs the config names -- output,
grad_input, grad_weight -- on the int8 MFMA: both operands are cast per row or per column (absmax, scale = amax / 127) on the fly, multiplied
in int32 and scaled back in one rounding (csrc/int8_train_kernels.hip).  No cast writes a transposed matrix: the casts leave their codes
where the elements lay and ops.int8_train_mm takes either operand in either layout, so the three GEMMs of a linear with W [N, K] are
    out          x row cast   x  W row cast      (flags 0, 0)
    grad_input   go row cast  x  W column cast   (flags 0, 1)
    grad_weightT x column cast x go column cast  (flags 1, 1), stored [K, N] and returned as its .T view, as the reference returns it
grad_output is cast once, rows and columns from the same two reads, when both gradients are int8.  A GEMM whose flag is False is torch's
bf16 matmul, as in the reference; the bias add and grad_bias are torch ops.

Left out, and refused by name: the FSDP2 hooks (fsdp_pre_all_gather, fsdp_post_all_gather), float16 and float32 inputs (bf16 directly or
through autocast), and in_features / out_features that are no multiple of 16."""
from dataclasses import dataclass
from typing import Optional, Union

import torch
import torch.nn.functional as F
import torch.utils._pytree as pytree
from torch import Tensor, nn

from ao_amd import ops

from ...quantization.config import AOBaseConfig
from ...quantization.quant_api import register_quantize_module_handler

aten = torch.ops.aten

_NO_FSDP = "int8 mixed-precision training on the MI355X has no FSDP2 / DTensor support: {} is not built"


@dataclass
class Int8MixedPrecisionTrainingConfig(AOBaseConfig):
    output: bool = True
    grad_input: bool = True
    grad_weight: bool = True
    module_swap: bool = False


int8_mixed_precision_training = Int8MixedPrecisionTrainingConfig  # for bc

_DEFAULT_CONFIG = Int8MixedPrecisionTrainingConfig()


class Int8MixedPrecisionTrainingLinearWeight(Tensor):
    """A wrapper of the high-precision weight whose F.linear runs the configured GEMMs in int8; every other op runs on the plain tensor."""

    @staticmethod
    @torch._dynamo.disable
    def __new__(cls, data: Tensor, config: Int8MixedPrecisionTrainingConfig):
        return Tensor._make_wrapper_subclass(cls, data.shape, data.stride(), data.storage_offset(), dtype=data.dtype, device=data.device)

    @torch._dynamo.disable
    def __init__(self, data: Tensor, config: Int8MixedPrecisionTrainingConfig):
        self._data = data
        self.config = config

    def __tensor_flatten__(self):
        return ["_data"], [self.config]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size=None, outer_stride=None):
        return cls(tensor_data_dict["_data"], *tensor_attributes)

    def __repr__(self):
        return f"{self.__class__.__name__}(data={self._data}, config={self.config})"

    def to_original(self):
        return self._data.clone()

    _PRESERVED = None  # the ops whose result stays wrapped (filled below)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is F.linear:
            input, weight = args[0], args[1]
            bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
            if torch.is_autocast_enabled("cuda"):
                dtype = torch.get_autocast_dtype("cuda")
                input, weight, bias = (x.to(dtype) if x is not None else x for x in (input, weight, bias))
            return _Int8MixedPrecisionTrainingLinearFunction.apply(input, weight, bias)
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)

    @classmethod
    def __torch_dispatch__(cls, func, types, args, kwargs=None):
        configs = []

        def unwrap(x):
            configs.append(x.config)
            assert x.config == configs[0]
            return x._data

        out = func(*pytree.tree_map_only(cls, unwrap, args), **pytree.tree_map_only(cls, unwrap, kwargs or {}))
        if func is aten.copy_.default:
            return args[0]  # the original object
        if func in cls._PRESERVED:
            return pytree.tree_map_only(Tensor, lambda x: cls(x, configs[0]), out)
        return out

    def fsdp_pre_all_gather(self, mesh, outer_size=None, outer_stride=None, module=None, mp_policy=None):
        raise NotImplementedError(_NO_FSDP.format("fsdp_pre_all_gather"))

    def fsdp_post_all_gather(self, all_gather_outputs, metadata, param_dtype, *, out=None):
        raise NotImplementedError(_NO_FSDP.format("fsdp_post_all_gather"))


Int8MixedPrecisionTrainingLinearWeight._PRESERVED = {
    aten.t.default, aten.detach.default, aten.empty_like.default, aten.new_zeros.default, aten.slice.Tensor, aten.view.default,
    aten.as_strided.default, aten._to_copy.default, aten._pin_memory.default, aten.split.Tensor, aten.clone.default,
}


class Int8MixedPrecisionTrainingLinear(nn.Linear):
    def __init__(self, *args, config: Int8MixedPrecisionTrainingConfig, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.config = config

    def forward(self, input: Tensor) -> Tensor:
        if torch.is_autocast_enabled("cuda"):
            input = input.to(torch.get_autocast_dtype("cuda"))
        return _Int8MixedPrecisionTrainingLinearFunction.apply(input, self.weight, self.bias, self.config)


def _dynamic_int8_mm(A: Tensor, B: Tensor) -> Tensor:
    """A [..., Kc] @ B [Kc, N] with A cast per row and B per column, the product scaled back in one rounding.  B is taken as it lies: a
    transposed view of a contiguous [N, Kc] tensor is cast along that tensor's rows, a contiguous B down its columns."""
    A2 = A.reshape(-1, A.shape[-1])
    a_q, a_s = ops.int8_train_quantize(A2)
    if B.t().is_contiguous():
        b_q, b_s = ops.int8_train_quantize(B.t())
        out = ops.int8_train_mm(a_q, b_q, a_s, b_s)
    else:
        b_q, b_s = ops.int8_train_quantize(B, rows=False, cols=True)
        out = ops.int8_train_mm(a_q, b_q, a_s, b_s, b_t=True)
    return out.view(*A.shape[:-1], out.shape[-1])


def _check(input: Tensor, weight: Tensor):
    if input.dtype != torch.bfloat16:
        raise NotImplementedError(f"Int8MixedPrecisionTraining: the input must be bfloat16, directly or through autocast, got {input.dtype} "
                                  "(float16 and float32 are not built)")
    n_w, k_w = weight.shape
    if k_w % 16 != 0 or n_w % 16 != 0:
        raise ValueError(f"Int8MixedPrecisionTraining: in_features={k_w} and out_features={n_w} must be multiples of 16")


class _Int8MixedPrecisionTrainingLinearFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input: Tensor, weight: Union[Int8MixedPrecisionTrainingLinearWeight, Tensor], bias: Optional[Tensor],
                config: Optional[Int8MixedPrecisionTrainingConfig] = None):
        if isinstance(weight, Int8MixedPrecisionTrainingLinearWeight):
            config = weight.config  # overrides the argument
            weight = weight._data
        config = _DEFAULT_CONFIG if config is None else config
        _check(input, weight)
        ctx.config = config
        ctx.save_for_backward(input, weight)
        ctx.bias = bias is not None
        weight = weight.to(input.dtype)
        if config.output:
            x = input.reshape(-1, weight.shape[1])
            x_q, x_s = ops.int8_train_quantize(x)
            w_q, w_s = ops.int8_train_quantize(weight)
            out = ops.int8_train_mm(x_q, w_q, x_s, w_s).view(*input.shape[:-1], weight.shape[0])
        else:
            out = input @ weight.T
        return out + bias if bias is not None else out

    @staticmethod
    def backward(ctx, grad_output):
        input, weight = ctx.saved_tensors
        weight = weight.to(input.dtype)
        config = ctx.config
        grad_input = grad_weight = grad_bias = None
        go = grad_output.reshape(-1, weight.shape[0])
        x = input.reshape(-1, weight.shape[1])
        int8_gi = ctx.needs_input_grad[0] and config.grad_input
        int8_gw = ctx.needs_input_grad[1] and config.grad_weight
        go_row = go_col = None
        if int8_gi or int8_gw:  # one cast of grad_output, both directions from the same two reads where both are wanted
            cast = ops.int8_train_quantize(go, rows=int8_gi, cols=int8_gw)
            go_row, go_col = (cast[:2] if int8_gi else None), (cast[-2:] if int8_gw else None)
        if ctx.needs_input_grad[0]:
            if int8_gi:
                w_q, w_s = ops.int8_train_quantize(weight, rows=False, cols=True)
                grad_input = ops.int8_train_mm(go_row[0], w_q, go_row[1], w_s, b_t=True).view(*grad_output.shape[:-1], weight.shape[1])
            else:
                grad_input = grad_output @ weight
        if ctx.needs_input_grad[1]:
            if int8_gw:
                x_q, x_s = ops.int8_train_quantize(x, rows=False, cols=True)
                grad_weight = ops.int8_train_mm(x_q, go_col[0], x_s, go_col[1], a_t=True, b_t=True).T
            else:
                grad_weight = go.T @ x
        if ctx.needs_input_grad[2] and ctx.bias:
            grad_bias = go.sum(0)
        return grad_input, grad_weight, grad_bias, None


@register_quantize_module_handler(Int8MixedPrecisionTrainingConfig)
def _int8_mixed_precision_training_transform(module: nn.Module, config: Int8MixedPrecisionTrainingConfig) -> nn.Module:
    n_w, k_w = module.weight.shape
    if k_w % 16 != 0 or n_w % 16 != 0:
        raise ValueError(f"Int8MixedPrecisionTrainingConfig: in_features={k_w} and out_features={n_w} must be multiples of 16")
    if config.module_swap:
        module.__class__ = Int8MixedPrecisionTrainingLinear
        module.config = config
        return module
    module.weight = nn.Parameter(Int8MixedPrecisionTrainingLinearWeight(module.weight.detach(), config), requires_grad=True)
    return module
