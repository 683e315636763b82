"""NF4Tensor, to_nf4, LinearNF4 and linear_nf4: the QLoRA base weight, MI355X-native.

Host-side mirror of torchao/quantization/quantize_/workflows/nf4/nf4_tensor.py
  * :580-1050   NF4Tensor (from_tensor, get_original_weight, flatten / unflatten, the two dispatch tables)
  * :1053-1079  LinearNF4, linear_nf4, to_nf4
for bfloat16 weights of at most two dimensions.  The reference's NF4 is eager PyTorch throughout: some 25 ops for the cast, a dozen for
get_original_weight, and every forward and backward of every base linear dequantizes the whole weight through them.  Here the cast is
two launches around torch's mean (ops.nf4_block_absmax, ops.nf4_quantize), get_original_weight is one (ops.nf4_dequantize), and the
forward at decode row counts is one launch that streams the fields once (ops.nf4_linear); above the route's seam the forward is
dequantize + F.linear, the reference's own chain.  The fields hold the reference's bytes (csrc/quant_math.h "NF4").

The torch-function table takes Tensor.to (a dtype dequantizes, a device moves the fields), .cpu, .cuda and F.linear (the bias is added
outside, as in the reference); the aten table takes detach, clone, _to_copy, to.dtype, t, mm and copy_ between tensors of equal
metadata.  Every other aten op raises NotImplementedError naming the op: split, slice, view, as_strided, new_zeros, cat, pinning, the
FSDP all-gather hooks, scatter, narrow and view_as -- the sharding surface of the reference -- are not implemented.  A tensor moved
to the CPU is storage only: there is no CPU fallback for the cast or the dequantize.
"""
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

from .. import ops

__all__ = ["NF4Tensor", "to_nf4", "LinearNF4", "linear_nf4", "SubclassTensorArgs", "NF4_TABLE"]

aten = torch.ops.aten

# reference :666-684
NF4_TABLE = [-1.0000, -0.6962, -0.5251, -0.3949, -0.2844, -0.1848, -0.0911, 0.0000,
             0.0796, 0.1609, 0.2461, 0.3379, 0.4407, 0.5626, 0.7230, 1.0000]

_INNER = ["quantized_data", "scaler_mean", "quantization_factor", "quantized_scalers", "nf4"]


class SubclassTensorArgs(NamedTuple):
    """reference :74-81"""
    original_shape: torch.Size
    original_strides: Tuple
    storage_offset: int
    dtype: torch.dtype
    device: torch.device
    requires_grad: bool


def _check_weight(name, tensor, block_size, scaler_block_size):
    """What to_nf4 refuses, by name, before any kernel is reached."""
    if not isinstance(tensor, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(tensor).__name__}")
    if tensor.dtype != torch.bfloat16:
        raise NotImplementedError(f"{name}: NF4 on MI355X takes bfloat16 weights, got {tensor.dtype}: cast explicitly "
                                  "(.to(torch.bfloat16)) if that rounding is acceptable")
    if tensor.dim() > 2:
        raise NotImplementedError(f"{name}: expect input tensor dim <= 2 but got dim = {tensor.dim()}")
    ops._nf4_format(name, tensor.numel(), block_size, scaler_block_size)


class NF4Tensor(torch.Tensor):
    """The reference's eight fields (:580-645): block_size, n_blocks, scaler_block_size, quantized_scalers int8 [n_blocks],
    quantization_factor bf16 [n_blocks / scaler_block_size], scaler_mean bf16 0-dim, quantized_data uint8 [numel / 2] (element 2i in
    the high nibble), nf4 the 16-entry table in bf16."""

    @staticmethod
    @torch._dynamo.disable
    def __new__(cls, tensor_meta, block_size, n_blocks, scaler_block_size, quantized_scalers, quantization_factor, scaler_mean,
                quantized_data, nf4):
        return torch.Tensor._make_wrapper_subclass(cls, tensor_meta.original_shape, tensor_meta.original_strides, tensor_meta.storage_offset,
                                                   dtype=tensor_meta.dtype, device=tensor_meta.device,
                                                   requires_grad=tensor_meta.requires_grad)

    @torch._dynamo.disable
    def __init__(self, tensor_meta, block_size, n_blocks, scaler_block_size, quantized_scalers, quantization_factor, scaler_mean,
                 quantized_data, nf4):
        self.block_size = block_size
        self.n_blocks = n_blocks
        self.scaler_block_size = scaler_block_size
        self.quantized_scalers = quantized_scalers
        self.quantization_factor = quantization_factor
        self.scaler_mean = scaler_mean
        self.quantized_data = quantized_data
        self.nf4 = nf4

    @classmethod
    @torch.no_grad()
    def from_tensor(cls, input_tensor: torch.Tensor, block_size: int, scaler_block_size: int):
        """reference :649-718: two launches and torch's mean in between (the only value of the format that depends on a summation order;
        the kernels read it through its pointer, no sync)."""
        _check_weight("NF4Tensor.from_tensor", input_tensor, block_size, scaler_block_size)
        x = input_tensor.detach().contiguous()
        absmax = ops.nf4_block_absmax(x, block_size)
        scaler_mean = absmax.mean()
        quantized_data, quantized_scalers, quantization_factor = ops.nf4_quantize(x, absmax, scaler_mean, block_size, scaler_block_size)
        nf4 = torch.tensor(NF4_TABLE, device=x.device, dtype=x.dtype)
        meta = SubclassTensorArgs(x.size(), x.stride(), x.storage_offset(), x.dtype, x.device, input_tensor.requires_grad)
        return cls(meta, block_size, x.numel() // block_size, scaler_block_size, quantized_scalers, quantization_factor, scaler_mean,
                   quantized_data, nf4)

    def _meta(self, **changes):
        meta = SubclassTensorArgs(self.size(), self.stride(), self.storage_offset(), self.dtype, self.device, self.requires_grad)
        return meta._replace(**changes)

    def _with_fields(self, fn, **meta_changes):
        """A new NF4Tensor over fn(field) for the five inner tensors."""
        f = {n: fn(getattr(self, n)) for n in _INNER}
        meta_changes.setdefault("device", f["quantized_data"].device)
        return NF4Tensor(self._meta(**meta_changes), self.block_size, self.n_blocks, self.scaler_block_size, f["quantized_scalers"],
                         f["quantization_factor"], f["scaler_mean"], f["quantized_data"], f["nf4"])

    def _is_transposed(self):
        return self.dim() == 2 and not self.is_contiguous()

    def get_original_weight(self) -> torch.Tensor:
        """reference :845-871, its bits, in one launch (ops.nf4_dequantize); the t() of a weight comes back as the t() of its values."""
        w = ops.nf4_dequantize(self.quantized_data, self.quantized_scalers, self.quantization_factor, self.scaler_mean, self.block_size,
                               self.scaler_block_size)
        if self._is_transposed():
            return w.view(self.shape[1], self.shape[0]).t()
        return w.view(self.shape)

    def __repr__(self):
        return f"NF4Tensor({tuple(self.shape)}, block_size={self.block_size}, scaler_block_size={self.scaler_block_size}, device={self.device})"

    def __str__(self):
        return f"NF4Tensor({self.shape}, {self.block_size})"

    def __tensor_flatten__(self):
        """reference :894-915"""
        ctx = {"block_size": self.block_size, "n_blocks": self.n_blocks, "scaler_block_size": self.scaler_block_size,
               "tensor_meta": self._meta()}
        return list(_INNER), ctx

    @staticmethod
    def __tensor_unflatten__(inner_tensors, metadata, outer_size, outer_stride):
        """reference :917-930"""
        assert len(inner_tensors) == 5, "Expected 5 inner tensors"
        return NF4Tensor(metadata["tensor_meta"], metadata["block_size"], metadata["n_blocks"], metadata["scaler_block_size"],
                         inner_tensors["quantized_scalers"], inner_tensors["quantization_factor"], inner_tensors["scaler_mean"],
                         inner_tensors["quantized_data"], inner_tensors["nf4"])

    @classmethod
    @torch._dynamo.disable
    def __torch_dispatch__(cls, func, types, args, kwargs=None):
        impl = NF4_OPS_TABLE.get(func)
        if impl is not None:
            return impl(func, args, kwargs or {})
        raise NotImplementedError(f"NF4Tensor dispatch: attempting to run {func}, this is not supported")

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        impl = NF4_TORCH_FUNCTIONS.get(func)
        if impl is not None:
            return impl(*args, **kwargs)
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)


def same_metadata(a, b):
    """reference :87-94"""
    return (isinstance(a, NF4Tensor) and isinstance(b, NF4Tensor) and a.block_size == b.block_size
            and a.scaler_block_size == b.scaler_block_size and a.n_blocks == b.n_blocks)


class LinearNF4(torch.autograd.Function):
    """reference :1053-1064.  forward: ops.nf4_linear on the tensor's own fields (the fused stream launch, or dequantize + F.linear, by
    the route); backward: grad_output @ dequantize(weight), the weight never has a gradient."""

    @staticmethod
    def forward(ctx, input: torch.Tensor, weight: NF4Tensor):
        from ..torch_ops import kernels

        if input.dtype != torch.bfloat16:
            raise NotImplementedError(f"linear_nf4: NF4 on MI355X takes bfloat16 activations, got {input.dtype}")
        if weight.dim() != 2 or weight._is_transposed():
            raise NotImplementedError(f"linear_nf4: the weight must be a contiguous 2-D NF4Tensor [N, K], got shape {tuple(weight.shape)}")
        ctx.save_for_backward(weight)
        n, k = weight.shape
        x2 = input.reshape(-1, input.shape[-1])
        y = kernels(x2).nf4_linear(x2, weight.quantized_data, weight.quantized_scalers, weight.quantization_factor, weight.scaler_mean, n, k,
                                   weight.block_size, weight.scaler_block_size)
        return y.reshape(*input.shape[:-1], n)

    @staticmethod
    def backward(ctx, grad_output):
        weight: NF4Tensor = ctx.saved_tensors[0]
        w = weight.get_original_weight()
        g2 = grad_output.reshape(-1, grad_output.shape[-1])
        return torch.mm(g2, w.to(grad_output.dtype)).reshape(*grad_output.shape[:-1], w.shape[1]), None


def linear_nf4(input: torch.Tensor, weight: NF4Tensor) -> torch.Tensor:
    """reference :1067-1074"""
    return LinearNF4.apply(input, weight)


def to_nf4(tensor, block_size: int = 64, scaler_block_size: int = 256):
    """reference :1077-1079"""
    return NF4Tensor.from_tensor(tensor, block_size, scaler_block_size)


# ---- the torch-function table (reference :1082-1145) ------------------------------------------------------------------------------------
NF4_TORCH_FUNCTIONS = {}
NF4_OPS_TABLE = {}


def implements_torch_function(torch_function):
    def decorator(func):
        NF4_TORCH_FUNCTIONS[torch_function] = func
        return func

    return decorator


def implements(aten_ops):
    def decorator(func):
        for op in aten_ops:
            NF4_OPS_TABLE[op] = func
        return func

    return decorator


@implements_torch_function(torch.Tensor.to)
def _function_to(*args, **kwargs):
    """reference :1094-1115: a dtype dequantizes, a device alone moves the fields"""
    tensor = args[0]
    device, dtype, non_blocking, convert_to_format = torch._C._nn._parse_to(*args[1:], **kwargs)
    if dtype is not None:
        return tensor.get_original_weight().to(device, dtype, non_blocking, memory_format=convert_to_format)
    return tensor._with_fields(lambda t: t.to(device=device, non_blocking=non_blocking))


@implements_torch_function(torch.Tensor.cpu)
def _function_cpu(*args, **kwargs):
    return args[0].to("cpu", *args[1:], **kwargs)


@implements_torch_function(torch.Tensor.cuda)
def _function_cuda(*args, **kwargs):
    return args[0]._with_fields(lambda t: t.cuda(*args[1:], **kwargs))


@implements_torch_function(F.linear)
def _function_linear(*args, **kwargs):
    """reference :1137-1145: the bias is added outside"""
    input, weight = args[0], args[1]
    bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
    out = LinearNF4.apply(input, weight)
    return out if bias is None else out + bias


# ---- the aten table (reference :186-204, :376-454) ------------------------------------------------------------------------------------------
@implements([aten.detach.default])
def _nf4_detach(func, args, kwargs):
    return args[0]._with_fields(lambda t: t.detach(), requires_grad=False)


@implements([aten.clone.default])
def _nf4_clone(func, args, kwargs):
    """(the reference dequantizes and casts again, :191-193: the same bytes)"""
    return args[0]._with_fields(lambda t: t.clone())


@implements([aten._to_copy.default])
def _nf4_to_copy(func, args, kwargs):
    """reference :376-384"""
    t, dtype, device = args[0], kwargs.get("dtype"), kwargs.get("device")
    if dtype is None:
        return t._with_fields(lambda f: f.to(device) if device is not None else f.clone())
    out = t.get_original_weight().to(dtype)
    return out if device is None else out.to(device)


@implements([aten.to.dtype])
def _nf4_to_dtype(func, args, kwargs):
    """reference :387-392"""
    return args[0].get_original_weight().to(args[1])


@implements([aten.t.default])
def _nf4_t(func, args, kwargs):
    """reference :395-417: metadata only, the fields are shared"""
    a = args[0]
    if a.dim() != 2:
        raise NotImplementedError(f"aten.t(NF4Tensor) with dim={a.dim()}")
    return a._with_fields(lambda f: f, original_shape=torch.Size((a.shape[1], a.shape[0])), original_strides=(a.stride(1), a.stride(0)))


@implements([aten.mm.default])
def _nf4_mm(func, args, kwargs):
    """reference :420-422: x @ weight.t() is linear_nf4(x, weight)"""
    x, wt = args[0], args[1]
    if not isinstance(wt, NF4Tensor) or isinstance(x, NF4Tensor) or not wt._is_transposed():
        raise NotImplementedError("aten.mm(NF4Tensor): only x @ weight.t() with a plain x and the t() of an [N, K] NF4Tensor is supported")
    return linear_nf4(x, wt.t())


@implements([aten.copy_.default])
def _nf4_copy_(func, args, kwargs):
    """reference :425-440, the base case only"""
    original, copy_in = args[0], args[1]
    if not same_metadata(original, copy_in):
        raise NotImplementedError("aten.copy_(NF4Tensor): only between NF4Tensors of equal block_size, scaler_block_size and n_blocks")
    for name in _INNER:
        getattr(original, name).copy_(getattr(copy_in, name))
    return original


torch.serialization.add_safe_globals([NF4Tensor, SubclassTensorArgs])
