"""Codebook (k-means) weight-only quantization, MI355X-native: CodebookWeightOnlyConfig, CodebookQuantizedTensor and the three ops.

Host-side mirror of torchao/prototype/quantization/codebook
  * codebook_ops.py:16-221              quantize_codebook, dequantize_codebook, choose_qparams_codebook
  * codebook_ops.py:224-359             _kmeans_greedy_init, fit_kmeans (single device)
  * codebook_quantized_tensor.py:26-308 CodebookQuantizedTensor, CodebookWeightOnlyConfig, the quantize_ handler
for 2-D bfloat16 weights, block_size (1, d) with d in {1, 2, 4, 8} and torch.uint4 / torch.uint8 codes (16 / 256 entries): 8, 4, 2 and
1 bit a weight.  The format is stated once, in csrc/quant_math.h ("Codebook"); DESIGN.md 4.35 has the kernels and the measurements.

An iteration of the reference's k-means is an addmm that writes a [blocks, k] fp32 score matrix, an argmax and an index_reduce_ whose
atomics funnel every block onto k rows; here it is ops.codebook_lloyd_step (two launches, the table in LDS, no score matrix, no global
atomics).  F.linear runs by ops.codebook_linear's route: at decode row counts one launch that streams the codes and gathers MFMA
operands from the table in LDS, else dequantize + F.linear, the reference's own chain.

Deviations from the reference, all named: uint4 codes are stored two a byte (block 2 i in the low nibble) in place of UintxTensor; the
assignment takes the LOWEST index among equal scores and fixes the order of the score's fused multiply-adds; everything the kernels
do not take is refused by name before any launch.  There is no CPU fallback.
"""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.nn.functional as F

from .. import ops
from ..quantization.config import AOBaseConfig
from ..quantization.quant_api import register_quantize_module_handler

__all__ = ["CodebookWeightOnlyConfig", "codebook_weight_only", "CodebookQuantizedTensor", "choose_qparams_codebook", "quantize_codebook",
           "dequantize_codebook"]

aten = torch.ops.aten

_ENTRIES = {torch.uint4: 16, torch.uint8: 256}


def _check_format(name, shape, dtype, block_size, scale_block_size, code_dtype):
    """What the format does not hold, by name and with the working alternative, before any launch.  -> (N, K, d, entries)"""
    if code_dtype not in _ENTRIES:
        raise NotImplementedError(f"{name}: code dtype {code_dtype} is not built: torch.uint1-3 and torch.uint5-7 need the reference's UintxTensor "
                                  "packing and torch.int32 a 65536-entry table that does not fit LDS; use torch.uint4 (16 entries) or torch.uint8 (256)")
    if dtype != torch.bfloat16:
        raise NotImplementedError(f"{name}: codebook weights on MI355X take bfloat16, got {dtype} (float16 and float32 are not built): cast "
                                  "explicitly (.to(torch.bfloat16)) if that rounding is acceptable")
    if len(shape) != 2:
        raise NotImplementedError(f"{name}: expected a 2-D weight [N, K], got {len(shape)}-D {tuple(shape)} (conv and embedding weights are not built)")
    block_size = tuple(block_size)
    if len(block_size) != 2 or block_size[0] != 1 or block_size[1] not in ops.CODEBOOK_BLOCK_WIDTHS:
        raise NotImplementedError(f"{name}: block_size {block_size} is not built: blocks are (1, d) with d in {ops.CODEBOOK_BLOCK_WIDTHS} "
                                  "(out-blocks taller than one row and wider blocks do not fit an MFMA operand of 8 k)")
    n, k = shape
    d = block_size[1]
    if k % d != 0:
        raise ValueError(f"{name}: K={k} must be divisible by the block width {d}")
    if not isinstance(scale_block_size, int) or scale_block_size < 1 or k % scale_block_size != 0:
        raise ValueError(f"{name}: input_features ({k}) must be divisible by scale_block_size ({scale_block_size})")
    if scale_block_size % d != 0:
        raise ValueError(f"{name}: scale_block_size ({scale_block_size}) must be a multiple of the block width {d}: a block has one scale")
    if code_dtype == torch.uint4 and (k // d) % 2 != 0:
        raise ValueError(f"{name}: K / d = {k // d} must be even for torch.uint4 codes (two a byte); use torch.uint8")
    return n, k, d, _ENTRIES[code_dtype]


def _scales_and_data(input_tensor, d, scale_block_size):
    """choose_qparams_codebook :190-212: the fp32 scales [N, K / sb, 1] and the k-means data [N K / d, d] = f32(W) / scales."""
    n, k = input_tensor.shape
    x = input_tensor.to(torch.float32).view(n, k // scale_block_size, scale_block_size)
    if d == 1:  # (the reference's quirk, kept: the SIGNED maximum)
        scales = x.max(dim=-1, keepdim=True).values
    else:
        scales = torch.linalg.vector_norm(x, dim=-1, keepdim=True)
    scales = torch.clamp(scales, min=1e-9)
    return scales, (x / scales).view(-1, d)


def _farthest_point_init(data: torch.Tensor, k: int) -> torch.Tensor:
    """The greedy initialisation of the reference's k-means (codebook_ops.py:224-243) in tensor ops, k short steps: entry 0 is row 0, each
    further entry the row farthest from the entries so far.  A row already chosen is at distance exactly 0 (r - 2 r + r in fp32)."""
    table = data.new_zeros(k, data.shape[1])
    norms = (data * data).sum(dim=1)
    far = torch.full_like(norms, torch.inf)
    for j in range(k):
        c = data[far.argmax()]
        table[j] = c
        torch.minimum(far, norms - 2 * (data @ c) + c.dot(c), out=far)
    return table


def _fit_kmeans(data, k, max_iter=200, check_every=10, rtol=1e-06, atol=1e-08):
    """fit_kmeans :247-344 on one device: one ops.codebook_lloyd_step an iteration; the allclose every check_every iterations is the only
    synchronisation."""
    clusters = _farthest_point_init(data, k)
    for i in range(max_iter):
        new_clusters, _ = ops.codebook_lloyd_step(data, clusters)
        if i % check_every == 0 and torch.allclose(new_clusters, clusters, rtol=rtol, atol=atol):
            break
        clusters = new_clusters
    return clusters


def _assign(data, codebook, n, code_dtype):
    codes = ops.codebook_assign(data, codebook.reshape(codebook.shape[0], -1).to(torch.float32)).view(n, -1)
    return ops.codebook_pack_u4(codes) if code_dtype == torch.uint4 else codes


@torch.no_grad()
def choose_qparams_codebook(input_tensor: torch.Tensor, block_size: Tuple[int, ...], scale_block_size: int, code_dtype: torch.dtype,
                            max_iter: int = 200, devices: Optional[List[torch.device]] = None):
    """reference codebook_ops.py:152-221 -> (codebook fp32 [k, 1, d], scales fp32 [N, K / sb, 1]).  input_tensor: the bf16 weight or, as
    the reference's from_float passes it, its float32 copy (checked as the bf16 weight it stands for); float16 is refused."""
    name = "choose_qparams_codebook"
    if devices is not None:
        raise NotImplementedError(f"{name}: devices= (data-parallel k-means over several GPUs) is not built: run on the weight's own device")
    dtype = torch.bfloat16 if input_tensor.dtype == torch.float32 else input_tensor.dtype
    _, _, d, k = _check_format(name, input_tensor.shape, dtype, block_size, scale_block_size, code_dtype)
    ops._require_gpu(name, input_tensor)
    scales, data = _scales_and_data(input_tensor, d, scale_block_size)
    return _fit_kmeans(data, k, max_iter).view(k, 1, d), scales


@torch.no_grad()
def quantize_codebook(input: torch.Tensor, codebook: torch.Tensor, scales: torch.Tensor, chunk_size: int = 1024,
                      code_dtype: torch.dtype = torch.uint4) -> torch.Tensor:
    """reference codebook_ops.py:16-95 in one launch (chunk_size is accepted and unused: no score matrix exists to bound) -> uint8 codes
    [N, K / d], or two a byte [N, K / (2 d)] for torch.uint4.  input: the bf16 weight or its float32 copy, as for choose_qparams_codebook; the
    codebook and scales in float32 (the unrounded pair) or bf16."""
    name = "quantize_codebook"
    dtype = torch.bfloat16 if input.dtype == torch.float32 else input.dtype
    if codebook.dim() != 3 or scales.dim() != 3 or scales.shape[1] < 1:
        raise ValueError(f"{name}: expected a codebook [k, 1, d] and scales [N, K / sb, 1], got {tuple(codebook.shape)} and {tuple(scales.shape)}")
    n, k_, d, k = _check_format(name, input.shape, dtype, tuple(codebook.shape[1:]), input.shape[-1] // scales.shape[1] if input.dim() == 2 else 1,
                                code_dtype)
    if codebook.shape[0] != k:
        raise ValueError(f"{name}: {code_dtype} codes index {k} entries, the codebook has {codebook.shape[0]}")
    ops._require_gpu(name, input, codebook, scales)
    data = (input.to(torch.float32).view(n, scales.shape[1], -1) / scales.to(torch.float32)).view(-1, d)
    return _assign(data, codebook, n, code_dtype)


@torch.no_grad()
def dequantize_codebook(codes: torch.Tensor, codebook: torch.Tensor, scales: torch.Tensor, output_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """reference codebook_ops.py:98-149 on the bf16 fields, one launch (ops.codebook_dequantize), then the cast the caller asks for"""
    assert output_dtype in [torch.float32, torch.float16, torch.bfloat16], f"Unsupported output dtype: {output_dtype}"
    return ops.codebook_dequantize(codes, codebook, scales).to(output_dtype)


class CodebookQuantizedTensor(torch.Tensor):
    """reference codebook_quantized_tensor.py:26-243: codes (uint8, two a byte for 16 entries), codebook bf16 [k, 1, d], scales bf16
    [N, K / sb, 1], block_size (1, d)."""

    @staticmethod
    def __new__(cls, codes, codebook, block_size, scales, shape, dtype=None, strides=None):
        kwargs = {"device": codes.device, "layout": codes.layout, "dtype": dtype, "requires_grad": False}
        if strides is not None:
            kwargs["strides"] = strides
        return torch.Tensor._make_wrapper_subclass(cls, shape, **kwargs)

    def __init__(self, codes, codebook, block_size, scales, shape, dtype=None, strides=None):
        self.codes = codes
        self.codebook = codebook
        self.block_size = tuple(block_size)
        self.scales = scales
        self._dtype = dtype

    def __repr__(self):
        return (f"{self.__class__.__name__}(shape={tuple(self.shape)}, block_size={self.block_size}, codebook_size={self.codebook.size(0)}, "
                f"scale_block_size={self.shape[-1] // self.scales.shape[1]}, device={self.device}, dtype={self.dtype})")

    def _quantization_type(self):
        return (f"shape={self.shape}, block_size={self.block_size}, codebook_size={self.codebook.size(0)}, device={self.device}, "
                f"code_dtype={self.codes.dtype}")

    def dequantize(self, output_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        return dequantize_codebook(self.codes, self.codebook, self.scales, output_dtype=self.dtype if output_dtype is None else output_dtype)

    def __tensor_flatten__(self):
        return ["codes", "codebook", "scales"], [self.block_size, self.shape, self.dtype]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        block_size, shape, dtype = tensor_attributes
        return cls(tensor_data_dict["codes"], tensor_data_dict["codebook"], block_size, tensor_data_dict["scales"],
                   shape if outer_size is None else outer_size, dtype=dtype, strides=outer_stride)

    @classmethod
    @torch.no_grad()
    def from_float(cls, input_tensor: torch.Tensor, block_size: Tuple[int, ...], code_dtype: torch.dtype, scale_block_size: int,
                   chunk_size: int = 1024):
        """reference :134-173.  The data f32(W) / scales is made ONCE and serves the k-means and the final assignment; both run on the
        fp32 table and scales, which are rounded to bf16 only afterwards, so the stored codes are those of the unrounded pair."""
        n, _, d, k = _check_format("CodebookQuantizedTensor.from_float", input_tensor.shape, input_tensor.dtype, block_size, scale_block_size,
                                   code_dtype)
        ops._require_gpu("CodebookQuantizedTensor.from_float", input_tensor)
        w = input_tensor.detach().contiguous()
        scales, data = _scales_and_data(w, d, scale_block_size)
        codebook = _fit_kmeans(data, k).view(k, 1, d)
        codes = _assign(data, codebook, n, code_dtype)
        return cls(codes, codebook.to(w.dtype), tuple(block_size), scales.to(w.dtype), w.shape, dtype=w.dtype)

    def to(self, *args, **kwargs):
        """reference :175-186: a device moves the fields (the dtype stays the weight's)"""
        device, dtype, _, _ = torch._C._nn._parse_to(*args, **kwargs)
        if dtype is not None and dtype != self.dtype:
            raise NotImplementedError(f"CodebookQuantizedTensor.to: the fields are bfloat16, got dtype={dtype}: dequantize(output_dtype) casts")
        device = self.device if device is None else device
        return self.__class__(self.codes.to(device), self.codebook.to(device), self.block_size, self.scales.to(device), self.shape, dtype=self.dtype)

    def detach(self):
        return self.__class__(self.codes.detach(), self.codebook.detach(), self.block_size, self.scales.detach(), self.shape, dtype=self.dtype)

    def requires_grad_(self, requires_grad=True):
        if requires_grad:
            raise NotImplementedError("CodebookQuantizedTensor: fine-tuning the table is not built; the weight is frozen")
        return self

    @property
    def dtype(self):
        return self._dtype  # (as the reference: avoids recursion through __torch_function__)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        """reference :199-215: the table below, else every instance among the arguments dequantizes first"""
        kwargs = kwargs or {}
        if func in CODEBOOK_TORCH_FUNCTIONS:
            return CODEBOOK_TORCH_FUNCTIONS[func](*args, **kwargs)
        with torch._C.DisableTorchFunctionSubclass():
            if getattr(func, "__name__", "") == "__get__" or func in _METADATA:  # shape, device, size(): the wrapper's own, no launch
                return func(*args, **kwargs)
            return func(*(arg.dequantize() if isinstance(arg, cls) else arg for arg in args), **kwargs)

    @classmethod
    def __torch_dispatch__(cls, func, types, args, kwargs=None):
        kwargs = kwargs or {}
        if func is aten.linear.default:
            return _linear(*args, **kwargs)
        if func is aten.detach.default:
            return args[0].detach()
        return func(*(arg.dequantize() if isinstance(arg, cls) else arg for arg in args), **kwargs)


def _linear(input, weight, bias=None):
    """F.linear / aten.linear on a CodebookQuantizedTensor weight, by ops.codebook_linear's route; the bias is added outside."""
    if not isinstance(weight, CodebookQuantizedTensor) or isinstance(input, CodebookQuantizedTensor):
        raise NotImplementedError("F.linear: only a plain activation with a CodebookQuantizedTensor weight is built")
    if input.dtype != torch.bfloat16:
        raise NotImplementedError(f"F.linear(CodebookQuantizedTensor): activations must be bfloat16, got {input.dtype} (float16 and float32 are not "
                                  "built): cast the activation, or multiply with weight.dequantize(dtype)")
    n, k = weight.shape
    x2 = input.reshape(-1, k)
    out = ops.codebook_linear(x2, weight.codes, weight.codebook, weight.scales).reshape(*input.shape[:-1], n)
    return out if bias is None else out + bias


CODEBOOK_TORCH_FUNCTIONS = {
    F.linear: _linear,
    torch.Tensor.detach: lambda tensor, *args, **kwargs: tensor.detach(),
    torch.Tensor.requires_grad_: lambda tensor, *args, **kwargs: tensor.requires_grad_(*args, **kwargs),
}
_METADATA = {torch.Tensor.size, torch.Tensor.dim, torch.Tensor.numel, torch.Tensor.stride, torch.Tensor.is_contiguous}


@dataclass
class CodebookWeightOnlyConfig(AOBaseConfig):
    """reference :266-270 (same fields and defaults)"""

    dtype: torch.dtype = torch.uint4
    block_size: Tuple[int, int] = (1, 1)
    scale_block_size: int = None


# for bc (reference :273-274)
codebook_weight_only = CodebookWeightOnlyConfig


@register_quantize_module_handler(CodebookWeightOnlyConfig)
def _codebook_weight_only_transform(module: torch.nn.Module, config: CodebookWeightOnlyConfig, *, parameter_name: str = "weight"):
    """reference :277-308, with its rule that a weight above 2^27 elements is left untouched (k-means is too unstable there)"""
    weight = getattr(module, parameter_name)
    if weight.numel() > 2**27:
        return module
    scale_block_size = weight.shape[-1] if config.scale_block_size is None else config.scale_block_size
    quantized_weight = CodebookQuantizedTensor.from_float(weight, block_size=config.block_size, code_dtype=config.dtype,
                                                          scale_block_size=scale_block_size)
    setattr(module, parameter_name, torch.nn.Parameter(quantized_weight, requires_grad=False))
    return module


torch.serialization.add_safe_globals([CodebookQuantizedTensor])
