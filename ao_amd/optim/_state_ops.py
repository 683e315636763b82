"""What the three optimizer-state subclasses share: copy_ in its three directions and dequantize on the two cast kernels
(ops.optim_quantize / ops.optim_dequantize), lerp on the dequantized value, and the structural ops that only rewrap the fields."""
import math

import torch
from torch.utils._python_dispatch import return_and_correct_aliasing

from .. import ops

aten = torch.ops.aten


def dequantize_state(x, output_dtype=None):
    """The fp32 values of a state (or those rounded once to bf16), in the state's shape."""
    kernel_dtype = torch.bfloat16 if output_dtype == torch.bfloat16 else torch.float32
    flat = ops.optim_dequantize(x.codes.reshape(-1) if x.codes.dim() != 1 else x.codes, x.scale, x._format(), x.block_size, x._qmap(), kernel_dtype)
    out = flat.view(tuple(x.shape))
    return out if output_dtype is None or output_dtype == kernel_dtype else out.to(output_dtype)


def register_state_ops(cls):
    """copy_, _to_copy, lerp.Scalar, view, detach and slice.Tensor for one state class (cls._rewrap builds a new wrapper over given fields)."""

    @cls.implements(aten.copy_.default)
    def _(func, types, args, kwargs):
        dst, src = args[0], args[1]
        if isinstance(dst, cls) and isinstance(src, cls):
            if dst._layout() != src._layout():
                raise ValueError(f"{cls.__name__}.copy_: the states differ in format: {dst._layout()} vs {src._layout()}")
            dst.codes.copy_(src.codes)
            dst.scale.copy_(src.scale)  # (the qmap of one format is one table)
        elif isinstance(dst, cls):
            if src.numel() != dst.numel():
                raise ValueError(f"{cls.__name__}.copy_: {src.numel()} values into a state of {dst.numel()}")
            if src.dtype not in (torch.float32, torch.bfloat16):
                src = src.float()
            ops.optim_quantize(src, dst._format(), dst.block_size, dst._qmap(), codes=dst.codes, scale=dst.scale)
        else:
            dst.copy_(src.dequantize())
        return dst

    @cls.implements(aten._to_copy.default)
    def _(func, types, args, kwargs):
        # only the appearance dtype and the device change
        x = args[0]
        device = kwargs.get("device", None)
        out = x._rewrap(*(t.to(device=device) for t in x._fields()), dtype=kwargs.get("dtype", x.dtype))
        return return_and_correct_aliasing(func, args, kwargs, out)

    @cls.implements(aten.lerp.Scalar)
    def _(func, types, args, kwargs):
        return func(*[a.dequantize() if isinstance(a, cls) else a for a in args], **kwargs)

    @cls.implements([aten.detach.default, aten.alias.default])
    def _(func, types, args, kwargs):
        x = args[0]
        return return_and_correct_aliasing(func, args, kwargs, x._rewrap(*(t.detach() for t in x._fields()), dtype=x.dtype))

    @cls.implements(aten.clone.default)
    def _(func, types, args, kwargs):
        x = args[0]
        return x._rewrap(*(t.clone() for t in x._fields()), dtype=x.dtype)

    @cls.implements(aten.contiguous.default)
    def _(func, types, args, kwargs):
        x = args[0]
        return x._rewrap(*(t.contiguous() for t in x._fields()), dtype=x.dtype)

    @cls.implements(aten.view.default)
    def _(func, types, args, kwargs):
        x, shape = args
        return x._view(shape)

    @cls.implements(aten.slice.Tensor)
    def _(func, types, args, kwargs):
        x, dim, start, end = args[:4]
        step = args[4] if len(args) > 4 else 1
        if dim != 0:
            raise ValueError("Only support aten.slice along the first dim")
        if step != 1:
            raise ValueError("Only support aten.slice with step=1")
        rows = x.shape[0]
        start = 0 if start is None else max(start + rows, 0) if start < 0 else min(start, rows)
        end = rows if end is None else max(end + rows, 0) if end < 0 else min(end, rows)
        stride = math.prod(x.shape[1:])
        if (start * stride) % x.block_size != 0 or (end * stride) % x.block_size != 0:
            raise ValueError(
                f"Invalid start or end for shape={tuple(x.shape)} and block_size={x.block_size}. "
                f"Make sure start and end align with block boundary. Received start={start}, end={end}."
            )
        return x._slice(start, end, stride)
