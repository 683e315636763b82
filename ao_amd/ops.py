"""Torch-facing wrappers over the C-ABI, one per reference op on the hot path.

Same argument meaning, output allocation ("allocate and return", inputs
borrowed) and error behaviour as the ops they replace; each docstring cites the
reference call site.  Tensors must live on the GPU ("cuda" == HIP device on
ROCm); there is no CPU fallback.
"""
import ctypes
from typing import Optional

import torch

from . import _lib

__all__ = [
    "convert_weight_to_int4pack",
    "unpack_int4pack",
    "weight_int4pack_mm",
    "int4_dequantize",
    "int4_quantize_tinygemm",
    "int4_plain_quantize",
    "int4_quantize_hqq",
    "int8_quantize_rowwise",
    "int8_scaled_mm",
    "int_mm",
    "fp8_quantize_rowwise",
    "fp8_scaled_mm",
    "mxfp8_quantize",
    "mxfp8_grouped_mm",
    "mxfp8_grouped_mm_wgrad",
    "mxfp8_mm_wgrad",
    "dynamic_linear_fits",
    "dynamic_linear_preferred",
    "int8_dynamic_linear",
    "fp8_dynamic_linear",
    "fused_pad_token_groups",
    "fused_unpad_token_groups",
    "mx_block_rearrange_2d_M_groups",
    "mx_to_blocked",
    "int8_linear",
    "fp8_linear",
    "mxfp8_quantize_colwise",
    "mxfp8_quantize_rowcol",
    "fp8_grouped_mm",
    "rowwise_amax",
    "int8_quantize_rowwise_amax",
    "fp8_quantize_rowwise_amax",
    "fp8_mm_f32",
    "int8_scale_epilogue",
    "fp8_scale_epilogue",
    "fp8_train_amax",
    "fp8_train_cast",
    "fp8_train_quantize_rowwise",
    "fp8_train_quantize_colwise_t",
    "fp8_train_quantize_both",
    "fp8_train_quantize_group_colwise_t",
    "fp8_train_quantize_colwise_t_3d",
    "fp8_grouped_mm_wgrad",
]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _on(dev):
    """Device guard for a launch: a no-op when `dev` is already current (torch.cuda.device() costs ~3 us per call, as much as a
    small decode kernel)."""
    return _NO_GUARD if dev.index == torch.cuda.current_device() else torch.cuda.device(dev)


def _require_gpu(name, *tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                f"{name}: expected all tensors on the GPU, got a tensor on {t.device} "
                "(the MI355X backend has no CPU fallback)"
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"{name}: tensors on different devices: {dev} vs {t.device}")
    return dev


def convert_weight_to_int4pack(w_u8: torch.Tensor, inner_k_tiles: int) -> torch.Tensor:
    """aten::_convert_weight_to_int4pack (call site: torchao/quantization/quantize_/
    workflows/int4/int4_tile_packed_to_4d_tensor.py:202).

    w_u8 uint8 [N, K/2] (even k in the high nibble) ->
    int32 [N/8, K/(inner_k_tiles*16), 32, inner_k_tiles/2].
    """
    dev = _require_gpu("convert_weight_to_int4pack", w_u8)
    if w_u8.dim() != 2:
        raise RuntimeError(f"convert_weight_to_int4pack: expected a 2-D tensor, got {w_u8.dim()}-D")
    if w_u8.dtype != torch.uint8:
        raise RuntimeError(f"convert_weight_to_int4pack: expected uint8, got {w_u8.dtype}")
    if not w_u8.is_contiguous():
        raise RuntimeError("convert_weight_to_int4pack: expected a contiguous tensor")
    if inner_k_tiles not in (2, 4, 8):
        raise RuntimeError(f"convert_weight_to_int4pack: innerKTiles must be 2, 4 or 8, got {inner_k_tiles}")
    n, kh = w_u8.shape
    k = kh * 2
    out = torch.empty(
        (n // 8, k // (inner_k_tiles * 16), 32, inner_k_tiles // 2), dtype=torch.int32, device=dev
    )
    with _on(dev):
        _lib.check(
            _lib.lib().ao_int4_convert_weight_to_int4pack(
                _ptr(w_u8), _ptr(out), n, k, inner_k_tiles, _stream()
            )
        )
    return out


def unpack_int4pack(qdata: torch.Tensor, inner_k_tiles: int = 8) -> torch.Tensor:
    """Inverse of convert_weight_to_int4pack: int32 4-D -> uint8 [N, K/2]."""
    dev = _require_gpu("unpack_int4pack", qdata)
    if qdata.dim() != 4 or qdata.dtype != torch.int32 or not qdata.is_contiguous():
        raise RuntimeError("unpack_int4pack: expected a contiguous 4-D int32 tensor")
    n = qdata.shape[0] * 8
    k = qdata.shape[1] * inner_k_tiles * 16
    out = torch.empty((n, k // 2), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(
            _lib.lib().ao_int4_unpack_int4pack(_ptr(qdata), _ptr(out), n, k, inner_k_tiles, _stream())
        )
    return out


def _int4_dims(name, qdata, scale_and_zero, group_size):
    if qdata.dim() != 4 or qdata.dtype != torch.int32:
        raise RuntimeError(f"{name}: mat2 must be a 4-D int32 tile-packed tensor")
    if qdata.shape[2] != 32 or qdata.shape[3] != 4:
        raise RuntimeError(f"{name}: mat2 must have shape [N/8, K/128, 32, 4] (innerKTiles = 8), got {tuple(qdata.shape)}")
    if not qdata.is_contiguous():
        raise RuntimeError(f"{name}: mat2 must be contiguous")
    n, k = qdata.shape[0] * 8, qdata.shape[1] * 128
    if group_size not in (32, 64, 128, 256):
        raise RuntimeError(f"{name}: qGroupSize must be one of 32, 64, 128, 256, got {group_size}")
    if scale_and_zero.dtype != torch.bfloat16 or scale_and_zero.dim() != 3:
        raise RuntimeError(f"{name}: qScaleAndZeros must be a 3-D bfloat16 tensor")
    if tuple(scale_and_zero.shape) != (k // group_size, n, 2):
        raise RuntimeError(
            f"{name}: qScaleAndZeros must have shape [K/g, N, 2] = {(k // group_size, n, 2)}, got {tuple(scale_and_zero.shape)}"
        )
    if not scale_and_zero.is_contiguous():
        raise RuntimeError(f"{name}: qScaleAndZeros must be contiguous")
    return n, k


def weight_int4pack_mm(
    x: torch.Tensor, qdata: torch.Tensor, group_size: int, scale_and_zero: torch.Tensor
) -> torch.Tensor:
    """aten::_weight_int4pack_mm(self, mat2, qGroupSize, qScaleAndZeros)
    (call site: int4_tile_packed_to_4d_tensor.py:287).

    x bf16 [M, K]; qdata int32 [N/8, K/128, 32, 4]; scale_and_zero bf16 [K/g, N, 2]
    -> bf16 [M, N].
    """
    dev = _require_gpu("weight_int4pack_mm", x, qdata, scale_and_zero)
    n, k = _int4_dims("weight_int4pack_mm", qdata, scale_and_zero, group_size)
    if x.dim() != 2:
        raise RuntimeError(f"weight_int4pack_mm: self must be 2-D, got {x.dim()}-D")
    if x.dtype != torch.bfloat16:
        raise RuntimeError(f"weight_int4pack_mm: self must be bfloat16, got {x.dtype}")
    if x.shape[1] != k:
        raise RuntimeError(f"weight_int4pack_mm: self has K={x.shape[1]} but mat2 has K={k}")
    if not x.is_contiguous():
        x = x.contiguous()
    m = x.shape[0]
    y = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    if m == 0:
        return y
    with _on(dev):
        _lib.check(
            _lib.lib().ao_int4_weight_int4pack_mm(
                _ptr(x), _ptr(qdata), _ptr(scale_and_zero), _ptr(y), m, n, k, group_size, _stream()
            )
        )
    return y


def int4_mm_pair(x0, qdata0, scale_and_zero0, x1, qdata1, scale_and_zero1, group_size: int):
    """Two weight_int4pack_mm calls of one shape in one launch (ao_int4_weight_int4pack_mm_pair): twin linears such as
    gate_proj / up_proj on the same activation (x0 may be x1).  Returns (y0, y1), the bits of the two single calls."""
    dev = _require_gpu("int4_mm_pair", x0, qdata0, scale_and_zero0, x1, qdata1, scale_and_zero1)
    n, k = _int4_dims("int4_mm_pair", qdata0, scale_and_zero0, group_size)
    if _int4_dims("int4_mm_pair", qdata1, scale_and_zero1, group_size) != (n, k):
        raise RuntimeError("int4_mm_pair: the two weights must have one N and K")
    for x in (x0, x1):
        if x.dim() != 2 or x.dtype != torch.bfloat16 or x.shape[1] != k:
            raise RuntimeError(f"int4_mm_pair: activations must be bfloat16 [M, {k}], got {x.dtype} {tuple(x.shape)}")
    if x0.shape[0] != x1.shape[0]:
        raise RuntimeError("int4_mm_pair: the two activations must have one M")
    x0 = x0 if x0.is_contiguous() else x0.contiguous()
    x1 = x1 if x1.is_contiguous() else x1.contiguous()
    m = x0.shape[0]
    y0 = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    y1 = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    if m == 0:
        return y0, y1
    with _on(dev):
        _lib.check(
            _lib.lib().ao_int4_weight_int4pack_mm_pair(
                _ptr(x0), _ptr(qdata0), _ptr(scale_and_zero0), _ptr(y0), _ptr(x1), _ptr(qdata1), _ptr(scale_and_zero1), _ptr(y1),
                m, n, k, group_size, _stream()
            )
        )
    return y0, y1


def int4_dequantize(qdata: torch.Tensor, scale_and_zero: torch.Tensor, group_size: int) -> torch.Tensor:
    """Packed int4 -> bf16 [N, K] with the reference's rounding sequence
    (torchao/quantization/utils.py:445-455, quant_primitives.py:999-1007)."""
    dev = _require_gpu("int4_dequantize", qdata, scale_and_zero)
    n, k = _int4_dims("int4_dequantize", qdata, scale_and_zero, group_size)
    w = torch.empty((n, k), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(
            _lib.lib().ao_int4_dequantize(_ptr(qdata), _ptr(scale_and_zero), _ptr(w), n, k, group_size, _stream())
        )
    return w


def int4_quantize_tinygemm(w: torch.Tensor, group_size: int):
    """Fused tinygemm weight prep (int4_tile_packed_to_4d_tensor.py:129-236):
    bf16 [N, K] (N % 16 == 0, K % 128 == 0) -> (qdata int32 [N/8, K/128, 32, 4],
    scale_and_zero bf16 [K/g, N, 2])."""
    dev = _require_gpu("int4_quantize_tinygemm", w)
    if w.dim() != 2 or w.dtype != torch.bfloat16:
        raise RuntimeError("int4_quantize_tinygemm: expected a 2-D bfloat16 tensor")
    if not w.is_contiguous():
        w = w.contiguous()
    n, k = w.shape
    qdata = torch.empty((n // 8, k // 128, 32, 4), dtype=torch.int32, device=dev)
    sz = torch.empty((k // max(group_size, 1), n, 2), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(
            _lib.lib().ao_int4_quantize_tinygemm(_ptr(w), _ptr(qdata), _ptr(sz), n, k, group_size, _stream())
        )
    return qdata, sz


def int4_quantize_hqq(w: torch.Tensor, group_size: int):
    """HQQ qparams + codes in the tinygemm format (Int4TilePackedTo4dTensor.from_hp with Int4ChooseQParamsAlgorithm.HQQ,
    int4_tile_packed_to_4d_tensor.py:149-236).  w bf16 [N, K] (N % 16 == 0, K % 128 == 0) ->
    (qdata int32 [N/8, K/128, 32, 4], scale_and_zero bf16 [K/g, N, 2]).  Synchronises the stream (the optimizer's early stop
    reads a global error every iteration, as the reference's does)."""
    dev = _require_gpu("int4_quantize_hqq", w)
    if w.dtype != torch.bfloat16 or w.dim() != 2:
        raise RuntimeError("int4_quantize_hqq: expected a 2-D bfloat16 tensor")
    w = w.contiguous()
    n, k = w.shape
    if n % 16 != 0 or k % 128 != 0 or group_size not in (32, 64, 128, 256) or k % group_size != 0:
        raise ValueError(f"int4_quantize_hqq: shape {tuple(w.shape)} / group_size {group_size} not supported (N % 16, K % 128, g 32|64|128|256)")
    lib = _lib.lib()
    ws = torch.empty((int(lib.ao_int4_hqq_workspace_bytes(n, k, group_size)),), dtype=torch.uint8, device=dev)
    nib = torch.empty((n, k // 2), dtype=torch.uint8, device=dev)
    sz = torch.empty((k // group_size, n, 2), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(lib.ao_int4_quantize_hqq(_ptr(w), _ptr(nib), _ptr(sz), _ptr(ws), n, k, group_size, _stream()))
    return convert_weight_to_int4pack(nib, 8), sz


def int4_plain_quantize(w: torch.Tensor, group_size: int, symmetric: bool = False):
    """Int4Tensor.from_hp's arithmetic, PLAIN packing (quantize_/workflows/int4/int4_tensor.py:130-186; mslk's
    int4_row_quantize_zp / int4_row_quantize + pack_int4 as restated by the reference, qat/fake_quantizer.py:148-190).
    w bf16 [N, K] -> (qdata uint8 [N, K/2] even k in the low nibble, scale bf16 [K/g, N], zero_point bf16 [K/g, N])."""
    dev = _require_gpu("int4_plain_quantize", w)
    if w.dtype != torch.bfloat16 or w.dim() != 2:
        raise RuntimeError("int4_plain_quantize: expected a 2-D bfloat16 tensor")
    w = w.contiguous()
    n, k = w.shape
    if group_size not in (32, 64, 128, 256) or k % 128 != 0 or k % group_size != 0:
        raise ValueError(f"int4_plain_quantize: group_size {group_size} / K={k} not supported (group 32|64|128|256, K % 128 == 0)")
    qdata = torch.empty((n, k // 2), dtype=torch.uint8, device=dev)
    scale = torch.empty((k // group_size, n), dtype=torch.bfloat16, device=dev)
    zero = torch.empty((k // group_size, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_int4_plain_quantize(_ptr(w), _ptr(qdata), _ptr(scale), _ptr(zero), n, k, group_size, int(bool(symmetric)),
                                                     _stream()))
    return qdata, scale, zero


# ---------------------------------------------------------------------------
# int8 dynamic activation x int8 weight
# ---------------------------------------------------------------------------
def _as_rows(name, x, dtype):
    if x.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {x.dtype}")
    if x.dim() != 2:
        raise RuntimeError(f"{name}: expected a 2-D tensor, got {x.dim()}-D")
    return x if x.is_contiguous() else x.contiguous()


def _int8_rows_and_pre(name, x, pre):
    """x as contiguous bf16 rows under the checks of the plain casts (pre is None) or, with an activation pre-scale, of the pre-scaled
    ones; and `pre` as its contiguous bf16 [K] vector."""
    if pre is None:
        return _as_rows(name, x, torch.bfloat16), None
    x = _sq_rows(name, x)
    return x, _sq_vector(name, "pre", pre, x.shape[1])


def _int8_quantize_rowwise(name, x, pre=None):
    """The per-row cast of x or, with `pre`, of x * pre (the product never written)."""
    dev = _require_gpu(name, x, pre)
    x, pre = _int8_rows_and_pre(name, x, pre)
    m, k = x.shape
    q = torch.empty((m, k), dtype=torch.int8, device=dev)
    s = torch.empty((m, 1), dtype=torch.float32, device=dev)
    with _on(dev):
        if pre is None:
            _lib.check(_lib.lib().ao_int8_quantize_rowwise(_ptr(x), _ptr(q), _ptr(s), m, k, _stream()))
        else:
            _lib.check(_lib.lib().ao_int8_quantize_rowwise_prescaled(_ptr(x), _ptr(pre), _ptr(q), _ptr(s), m, k, _stream()))
    return q, s


def int8_quantize_rowwise(x: torch.Tensor):
    """Int8Tensor.from_hp(x, PerRow()) (symmetric, eps = fp32 eps):
    torchao/quantization/quantize_/workflows/int8/int8_tensor.py:176-248.
    x bf16 [M, K] -> (qdata int8 [M, K], scale fp32 [M, 1])."""
    return _int8_quantize_rowwise("int8_quantize_rowwise", x)


def int8_scaled_mm(xq, x_scale, wq, w_scale, bias=None):
    """_int_scaled_matmul + weight-scale epilogue of the Int8Tensor linear
    (int8/kernels.py:114-144, int8_tensor.py:305-359).
    xq int8 [M, K]; x_scale fp32 [M(,1)]; wq int8 [N, K]; w_scale fp32 [N(,1)];
    bias bf16 [N] or None -> bf16 [M, N]."""
    dev = _require_gpu("int8_scaled_mm", xq, x_scale, wq, w_scale, bias)
    xq = _as_rows("int8_scaled_mm", xq, torch.int8)
    wq = _as_rows("int8_scaled_mm", wq, torch.int8)
    m, k = xq.shape
    n, k2 = wq.shape
    if k != k2:
        raise RuntimeError(f"int8_scaled_mm: K mismatch {k} vs {k2}")
    x_scale = x_scale.reshape(-1).to(torch.float32).contiguous()
    w_scale = w_scale.reshape(-1).to(torch.float32).contiguous()
    if x_scale.numel() != m or w_scale.numel() != n:
        raise RuntimeError("int8_scaled_mm: scales must be per-row ([M] and [N])")
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
        if bias.numel() != n:
            raise RuntimeError("int8_scaled_mm: bias must have N elements")
    y = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(
            _lib.lib().ao_int8_scaled_mm(
                _ptr(xq), _ptr(x_scale), _ptr(wq), _ptr(w_scale), _ptr(bias), _ptr(y), m, n, k, _stream()
            )
        )
    return y


def int_mm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """aten::_int_mm(self int8 [M, K], mat2 int8 [K, N]) -> int32 [M, N]
    (call sites: int8/kernels.py:38-40,70).  mat2 is expected K-major (the
    `.t()` of a row-major [N, K] weight, as the reference passes it); other
    layouts are made so with one copy."""
    dev = _require_gpu("int_mm", a, b)
    a = _as_rows("int_mm", a, torch.int8)
    if b.dtype != torch.int8 or b.dim() != 2:
        raise RuntimeError("int_mm: mat2 must be a 2-D int8 tensor")
    if a.shape[1] != b.shape[0]:
        raise RuntimeError(f"int_mm: shapes {tuple(a.shape)} and {tuple(b.shape)} cannot be multiplied")
    b_t = b.t()
    if not b_t.is_contiguous():
        b_t = b_t.contiguous()
    m, k = a.shape
    n = b_t.shape[0]
    c = torch.empty((m, n), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_int8_int_mm(_ptr(a), _ptr(b_t), _ptr(c), m, n, k, _stream()))
    return c


# ---------------------------------------------------------------------------
# float8 e4m3fn rowwise
# ---------------------------------------------------------------------------
def fp8_quantize_rowwise(x: torch.Tensor):
    """Float8Tensor.from_hp(x, float8_e4m3fn, PerRow())
    (quantize_/workflows/float8/float8_tensor.py:167-253).
    x bf16 [M, K] -> (qdata float8_e4m3fn [M, K], scale fp32 [M, 1])."""
    dev = _require_gpu("fp8_quantize_rowwise", x)
    x = _as_rows("fp8_quantize_rowwise", x, torch.bfloat16)
    m, k = x.shape
    q = torch.empty((m, k), dtype=torch.uint8, device=dev)
    s = torch.empty((m, 1), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_quantize_rowwise(_ptr(x), _ptr(q), _ptr(s), m, k, _stream()))
    return q.view(torch.float8_e4m3fn), s


def _fp8_bytes(name, t):
    if t.dtype == torch.float8_e4m3fn:
        t = t.view(torch.uint8)
    elif t.dtype != torch.uint8:
        raise RuntimeError(f"{name}: expected float8_e4m3fn data, got {t.dtype}")
    return t


def fp8_scaled_mm(a, b, scale_a, scale_b, bias=None):
    """aten::_scaled_mm with rowwise scales (torchao/float8/inference.py:104-123),
    out_dtype bf16.  a e4m3 [M, K] row-major; b e4m3 [K, N] column-major (i.e. the
    `.t()` of a row-major [N, K] weight); scale_a fp32 [M, 1]; scale_b fp32 [1, N]."""
    dev = _require_gpu("fp8_scaled_mm", a, b, scale_a, scale_b, bias)
    a = _fp8_bytes("fp8_scaled_mm", a)
    b = _fp8_bytes("fp8_scaled_mm", b)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0]:
        raise RuntimeError(f"fp8_scaled_mm: shapes {tuple(a.shape)} and {tuple(b.shape)} cannot be multiplied")
    if not a.is_contiguous():
        a = a.contiguous()
    b_t = b.t()
    if not b_t.is_contiguous():
        b_t = b_t.contiguous()
    m, k = a.shape
    n = b_t.shape[0]
    scale_a = scale_a.reshape(-1).to(torch.float32).contiguous()
    scale_b = scale_b.reshape(-1).to(torch.float32).contiguous()
    if scale_a.numel() != m or scale_b.numel() != n:
        raise RuntimeError("fp8_scaled_mm: only rowwise scaling is implemented (scale_a [M,1], scale_b [1,N])")
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
        if bias.numel() != n:
            raise RuntimeError("fp8_scaled_mm: bias must have N elements")
    y = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(
            _lib.lib().ao_fp8_scaled_mm(
                _ptr(a), _ptr(b_t), _ptr(scale_a), _ptr(scale_b), _ptr(bias), _ptr(y), m, n, k, _stream()
            )
        )
    return y


# ---------------------------------------------------------------------------
# K-sharded (row-parallel) 8-bit linears: building blocks (include/ao_mi355.h, last section)
# ---------------------------------------------------------------------------
def _strided_rows(name, x):
    """bf16 [M, K] whose rows are K-contiguous; a column slice of a wider row-major tensor is taken as is (row stride)."""
    if x.dtype != torch.bfloat16 or x.dim() != 2:
        raise RuntimeError(f"{name}: expected a 2-D bfloat16 tensor, got {x.dim()}-D {x.dtype}")
    if x.shape[1] % 8 != 0:
        raise ValueError(f"{name}: K={x.shape[1]} must be a multiple of 8")
    ok = x.stride(1) == 1 and x.stride(0) >= x.shape[1] and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0
    if not ok:
        x = x.contiguous()
        if x.data_ptr() % 16 != 0:  # a single row is "contiguous" wherever it starts
            x = x.clone()
    return x, (x.stride(0) if x.shape[0] > 1 else x.shape[1])  # (the stride of at most one row is never used)


def rowwise_amax(x: torch.Tensor) -> torch.Tensor:
    """max |x| per row of a bf16 [M, K] matrix (fp32 [M]): the local half of a full-K activation scale."""
    dev = _require_gpu("rowwise_amax", x)
    x, ldx = _strided_rows("rowwise_amax", x)
    m, k = x.shape
    out = torch.empty((m,), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_rowwise_amax(_ptr(x), ldx, _ptr(out), m, k, _stream()))
    return out


def _quantize_rowwise_amax(name, fn, x, amax, qdtype):
    dev = _require_gpu(name, x, amax)
    x, ldx = _strided_rows(name, x)
    m, k = x.shape
    amax = amax.reshape(-1).to(torch.float32).contiguous()
    if amax.numel() != m:
        raise RuntimeError(f"{name}: amax must have one entry per row ({m}), got {amax.numel()}")
    q = torch.empty((m, k), dtype=qdtype, device=dev)
    s = torch.empty((m, 1), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(fn(_ptr(x), ldx, _ptr(amax), _ptr(q), _ptr(s), m, k, _stream()))
    return q, s


def int8_quantize_rowwise_amax(x: torch.Tensor, amax: torch.Tensor):
    """Int8Tensor.from_hp arithmetic (int8_tensor.py:191-230) on a K shard of the activation, with the rows' amax over the
    full K given: the shard of the unsharded qdata, and the unsharded scale."""
    return _quantize_rowwise_amax("int8_quantize_rowwise_amax", _lib.lib().ao_int8_quantize_rowwise_amax, x, amax, torch.int8)


def fp8_quantize_rowwise_amax(x: torch.Tensor, amax: torch.Tensor):
    """Float8Tensor.from_hp arithmetic (float8_tensor.py:167-253) on a K shard, amax over the full K given."""
    q, s = _quantize_rowwise_amax("fp8_quantize_rowwise_amax", _lib.lib().ao_fp8_quantize_rowwise_amax, x, amax, torch.uint8)
    return q.view(torch.float8_e4m3fn), s


def fp8_mm_f32(a, b):
    """Unscaled e4m3 [M, K] @ e4m3 [K, N] (column-major, the `.t()` of a row-major [N, K] weight) -> fp32 [M, N]: the
    accumulator of aten::_scaled_mm before its scale epilogue."""
    dev = _require_gpu("fp8_mm_f32", a, b)
    a = _fp8_bytes("fp8_mm_f32", a)
    b = _fp8_bytes("fp8_mm_f32", b)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0]:
        raise RuntimeError(f"fp8_mm_f32: shapes {tuple(a.shape)} and {tuple(b.shape)} cannot be multiplied")
    if not a.is_contiguous():
        a = a.contiguous()
    b_t = b.t()
    if not b_t.is_contiguous():
        b_t = b_t.contiguous()
    m, k = a.shape
    n = b_t.shape[0]
    c = torch.empty((m, n), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_mm_f32(_ptr(a), _ptr(b_t), _ptr(c), m, n, k, _stream()))
    return c


def _scale_epilogue(name, fn, acc, acc_dtype, row_scale, col_scale, bias):
    dev = _require_gpu(name, acc, row_scale, col_scale, bias)
    if acc.dtype != acc_dtype or acc.dim() != 2:
        raise RuntimeError(f"{name}: expected a 2-D {acc_dtype} accumulator, got {acc.dim()}-D {acc.dtype}")
    acc = acc.contiguous()
    m, n = acc.shape
    row_scale = row_scale.reshape(-1).to(torch.float32).contiguous()
    col_scale = col_scale.reshape(-1).to(torch.float32).contiguous()
    if row_scale.numel() != m or col_scale.numel() != n:
        raise RuntimeError(f"{name}: scales must be per-row ([M] and [N])")
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
        if bias.numel() != n:
            raise RuntimeError(f"{name}: bias must have N elements")
    y = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(fn(_ptr(acc), _ptr(row_scale), _ptr(col_scale), _ptr(bias), _ptr(y), m, n, _stream()))
    return y


def int8_scale_epilogue(acc, x_scale, w_scale, bias=None):
    """bf16(bf16(acc * x_scale[m]) * w_scale[n] (+ bias)) over int32 accumulators (int8_tensor.py:315-359)."""
    return _scale_epilogue("int8_scale_epilogue", _lib.lib().ao_int8_scale_epilogue, acc, torch.int32, x_scale, w_scale, bias)


def fp8_scale_epilogue(acc, scale_a, scale_b, bias=None):
    """bf16(acc * scale_a[m] * scale_b[n] (+ bias)) over fp32 accumulators (float8/inference.py:104-123)."""
    return _scale_epilogue("fp8_scale_epilogue", _lib.lib().ao_fp8_scale_epilogue, acc, torch.float32, scale_a, scale_b, bias)


# ---- granularity / mapping variants of the dynamic-activation formats (PerTensor; int8 ASYMMETRIC activations) ----------
def _tensor_amax_rows(x):
    """[M] fp32 filled with max |x| over the WHOLE matrix (PerTensor granularity: block_size = shape)."""
    return rowwise_amax(x).amax().expand(x.shape[0])


def int8_quantize_tensorwise(x: torch.Tensor):
    """Int8Tensor.from_hp(x, PerTensor()) (int8_tensor.py:191-230 with block_size = shape): bf16 [M, K] ->
    (qdata int8 [M, K], scale fp32 [1, 1])."""
    q, s = int8_quantize_rowwise_amax(x, _tensor_amax_rows(x))
    return q, s[:1].reshape(1, 1)


def fp8_quantize_tensorwise(x: torch.Tensor):
    """Float8Tensor.from_hp(x, e4m3, PerTensor()) (float8_tensor.py:167-253 with block_size = shape): bf16 [M, K] ->
    (qdata e4m3fn [M, K], scale fp32 [1, 1])."""
    q, s = fp8_quantize_rowwise_amax(x, _tensor_amax_rows(x))
    return q, s[:1].reshape(1, 1)


# ---------------------------------------------------------------------------
# float8 TRAINING casts (torchao.float8): scale = f32(448 / max(f64(amax), 1e-12)), q = e4m3(clamp(f32(x) * scale)), and the
# reciprocal the GEMM takes.  Codes come back as float8_e4m3fn, scales as fp32 column vectors; the GEMM is fp8_scaled_mm.
# ---------------------------------------------------------------------------
def _fp8_train_rows(name, x, transposed=False):
    x = _as_rows(name, x, torch.bfloat16)
    r, c = x.shape
    if c % 16 != 0:
        raise ValueError(f"{name}: C={c} must be a multiple of 16")
    if transposed and r % 16 != 0:
        raise ValueError(f"{name}: R={r} must be a multiple of 16 for the transposed output (its rows are the GEMM's K)")
    return x, r, c


def _fp8_train_amax_arg(name, what, amax, n, dev):
    """An amax for the cast: one per row / column (n entries, stride 1) or one for the tensor (a single entry, stride 0)."""
    if amax.device != dev or amax.dtype != torch.float32:
        raise RuntimeError(f"{name}: {what} must be a float32 tensor on {dev}, got {amax.dtype} on {amax.device}")
    amax = amax.reshape(-1).contiguous()
    if amax.numel() == 1:
        return amax, 0
    if amax.numel() != n:
        raise RuntimeError(f"{name}: {what} must have {n} entries or one, got {amax.numel()}")
    return amax, 1


def fp8_train_amax(x: torch.Tensor, rows: bool = True, cols: bool = False):
    """tensor_to_amax (torchao/float8/float8_utils.py:56-82) along either or both axes in one read of x: bf16 [R, C] ->
    (row_amax fp32 [R] = max |x| over dim -1, or None; col_amax fp32 [C] = max |x| over dim 0, or None).  The whole tensor's amax is
    `row_amax.amax()`."""
    dev = _require_gpu("fp8_train_amax", x)
    x, r, c = _fp8_train_rows("fp8_train_amax", x)
    if not (rows or cols):
        raise ValueError("fp8_train_amax: neither rows nor cols asked for")
    alloc = torch.zeros if r == 0 or c == 0 else torch.empty  # (an empty matrix launches nothing: its maxima are 0)
    ra = alloc((r,), dtype=torch.float32, device=dev) if rows else None
    ca = alloc((c,), dtype=torch.float32, device=dev) if cols else None
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_train_amax(_ptr(x), _ptr(ra), _ptr(ca), r, c, _stream()))
    return ra, ca


def fp8_train_cast(x: torch.Tensor, row_amax: Optional[torch.Tensor] = None, col_amax: Optional[torch.Tensor] = None, pow2: bool = False):
    """hp_tensor_and_scale_to_float8 on the scale of amax_to_scale (float8_training_tensor.py:130-188, float8_utils.py:31-53) for either
    or both directions in one read of x.  x bf16 [R, C] -> (rows, cols):
      rows = (q e4m3fn [R, C], scale fp32 [R, 1], inv_scale fp32 [R, 1]) from row_amax, None without it;
      cols = (q_t e4m3fn [C, R], scale fp32 [C, 1], inv_scale fp32 [C, 1]) from col_amax, None without it: the cast along dim 0, stored
             transposed.
    An amax with ONE entry is the whole tensor's (TENSORWISE): the scale vectors are then filled with the one scale, which is the vector
    fp8_scaled_mm takes (float8_ops.py:356-359).  pow2: round_scales_to_power_of_2."""
    name = "fp8_train_cast"
    dev = _require_gpu(name, x, row_amax, col_amax)
    if row_amax is None and col_amax is None:
        raise ValueError(f"{name}: neither row_amax nor col_amax given")
    x, r, c = _fp8_train_rows(name, x, transposed=col_amax is not None)
    f32 = dict(dtype=torch.float32, device=dev)
    ra = rs = q = s = inv = ca = cs = qt = st = invt = None
    if row_amax is not None:
        ra, rs = _fp8_train_amax_arg(name, "row_amax", row_amax, r, dev)
        q, s, inv = torch.empty((r, c), dtype=torch.uint8, device=dev), torch.empty((r, 1), **f32), torch.empty((r, 1), **f32)
    if col_amax is not None:
        ca, cs = _fp8_train_amax_arg(name, "col_amax", col_amax, c, dev)
        qt, st, invt = torch.empty((c, r), dtype=torch.uint8, device=dev), torch.empty((c, 1), **f32), torch.empty((c, 1), **f32)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_train_cast(_ptr(x), _ptr(ra), rs or 0, _ptr(ca), cs or 0, int(bool(pow2)), _ptr(q), _ptr(s), _ptr(inv),
                                                _ptr(qt), _ptr(st), _ptr(invt), r, c, _stream()))
    return ((q.view(torch.float8_e4m3fn), s, inv) if q is not None else None,
            (qt.view(torch.float8_e4m3fn), st, invt) if qt is not None else None)


def fp8_train_quantize_rowwise(x: torch.Tensor, pow2: bool = False):
    """hp_tensor_to_float8_dynamic(x, e4m3, AXISWISE, axiswise_dim=-1) (float8_scaling_utils.py:29-72) as ONE launch: bf16 [R, C] ->
    (q e4m3fn [R, C], scale fp32 [R, 1], inv_scale fp32 [R, 1]); the bytes of fp8_train_amax + fp8_train_cast."""
    dev = _require_gpu("fp8_train_quantize_rowwise", x)
    x, r, c = _fp8_train_rows("fp8_train_quantize_rowwise", x)
    q = torch.empty((r, c), dtype=torch.uint8, device=dev)
    s = torch.empty((r, 1), dtype=torch.float32, device=dev)
    inv = torch.empty((r, 1), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_train_quantize_rowwise(_ptr(x), _ptr(q), _ptr(s), _ptr(inv), int(bool(pow2)), r, c, _stream()))
    return q.view(torch.float8_e4m3fn), s, inv


def fp8_train_quantize_colwise_t(x: torch.Tensor, pow2: bool = False, amax: Optional[torch.Tensor] = None):
    """hp_tensor_to_float8_dynamic(x, e4m3, AXISWISE, axiswise_dim=0), stored transposed: bf16 [R, C] -> (q_t e4m3fn [C, R], scale fp32
    [C, 1], inv_scale fp32 [C, 1]) -- the K-contiguous operand of a GEMM that contracts x's dim 0.  Two launches: amax, then cast.
    `amax` (one entry): the whole tensor's, for a TENSORWISE cast in this layout; the amax launch is then skipped."""
    if amax is None:
        amax = fp8_train_amax(x, rows=False, cols=True)[1]
    return fp8_train_cast(x, None, amax, pow2)[1]


def fp8_train_quantize_both(x: torch.Tensor, pow2: bool = False):
    """Both axiswise casts of x in two passes over it (one amax launch, one cast launch): bf16 [R, C] ->
    ((q, scale, inv_scale) of fp8_train_quantize_rowwise, (q_t, scale, inv_scale) of fp8_train_quantize_colwise_t), the same bytes."""
    ra, ca = fp8_train_amax(x, rows=True, cols=True)
    return fp8_train_cast(x, ra, ca, pow2)


def _offs_arg(name, offs, dev):
    if offs.dtype != torch.int32 or offs.dim() != 1 or offs.numel() < 1:
        raise RuntimeError(f"{name}: offs must be int32 [E], got {offs.dtype} {tuple(offs.shape)}")
    return offs.contiguous()


def fp8_train_quantize_group_colwise_t(x: torch.Tensor, offs: torch.Tensor, pow2: bool = True):
    """torch_to_float8_per_group_colwise (torchao/prototype/moe_training/utils.py:20-86; kernels/jagged_float8_scales.py:221-252), stored
    transposed: x bf16 [R, C], offs int32 [E] (cumulative group ends along R, multiples of 16, non-decreasing, within [0, R]; not validated)
    -> (q_t e4m3fn [C, R], scale fp32 [E, C], inv_scale fp32 [E, C]): one scale per column and token group, the amax over the group's rows.
    An empty group gets the scale of a zero amax; rows at or past offs[-1] belong to no group and get code 0."""
    name = "fp8_train_quantize_group_colwise_t"
    dev = _require_gpu(name, x, offs)
    x, r, c = _fp8_train_rows(name, x, transposed=True)
    offs = _offs_arg(name, offs, dev)
    e = offs.numel()
    qt = torch.empty((c, r), dtype=torch.uint8, device=dev)
    if r == 0 or c == 0:  # nothing is launched: every group is empty
        s = torch.full((e, c), 448.0 / 1e-12, dtype=torch.float32, device=dev)
        if pow2:
            s = (s.view(torch.int32) & -0x800000).view(torch.float32)
        return qt.view(torch.float8_e4m3fn), s, s.reciprocal()
    s = torch.empty((e, c), dtype=torch.float32, device=dev)
    inv = torch.empty((e, c), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_train_quantize_group_colwise_t(_ptr(x), _ptr(offs), _ptr(qt), _ptr(s), _ptr(inv), int(bool(pow2)), r, c, e,
                                                                    _stream()))
    return qt.view(torch.float8_e4m3fn), s, inv


def fp8_train_quantize_colwise_t_3d(w: torch.Tensor, pow2: bool = True):
    """torch_to_3d_rowwise_float8_transpose_rhs (torchao/prototype/moe_training/utils.py:156-189) of w.transpose(-2, -1): w bf16 [E, R, C]
    -> (q_t e4m3fn [E, C, R], scale fp32 [E, C], inv_scale fp32 [E, C]), the amax along R per expert; expert e's output is the bytes of
    fp8_train_quantize_colwise_t(w[e], pow2)."""
    name = "fp8_train_quantize_colwise_t_3d"
    dev = _require_gpu(name, w)
    if w.dtype != torch.bfloat16 or w.dim() != 3:
        raise RuntimeError(f"{name}: expected a 3-D bfloat16 tensor, got {w.dtype} {tuple(w.shape)}")
    w = w.contiguous()
    e, r, c = w.shape
    if c % 16 != 0 or r % 16 != 0:
        raise ValueError(f"{name}: R={r} and C={c} must be multiples of 16")
    qt = torch.empty((e, c, r), dtype=torch.uint8, device=dev)
    s = torch.empty((e, c), dtype=torch.float32, device=dev)
    inv = torch.empty((e, c), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_train_quantize_colwise_t_3d(_ptr(w), _ptr(qt), _ptr(s), _ptr(inv), int(bool(pow2)), e, r, c, _stream()))
    return qt.view(torch.float8_e4m3fn), s, inv


def fp8_grouped_mm_wgrad(g_t, g_inv, x_t, x_inv, offs, N: int, K: int):
    """The weight gradient of the float8 rowwise grouped mm (torchao/prototype/moe_training/fp8_grouped_mm.py:282-319) on the jagged casts
    of grad_out [M, N] and x [M, K] (fp8_train_quantize_group_colwise_t): g_t e4m3 [N, M], g_inv fp32 [E, N], x_t e4m3 [K, M], x_inv fp32
    [E, K], offs int32 [E] or None (one group of every token) -> bf16 [E, N, K] with
    out[e] = bf16((g_t[:, rows of e] @ x_t[:, rows of e]^T) * g_inv[e][:, None] * x_inv[e][None, :]); fp32 accumulation.  Any offsets; an
    empty group gives zeros."""
    name = "fp8_grouped_mm_wgrad"
    dev = _require_gpu(name, g_t, g_inv, x_t, x_inv, offs)
    n, k = int(N), int(K)
    g, x = _fp8_bytes(name, g_t), _fp8_bytes(name, x_t)
    if n <= 0 or k <= 0 or g.dim() != 2 or x.dim() != 2 or g.shape[0] != n or x.shape[0] != k or g.shape[1] != x.shape[1]:
        raise RuntimeError(f"{name}: g_t must be [N={n}, M] and x_t [K={k}, M], got {tuple(g_t.shape)} and {tuple(x_t.shape)}")
    m = g.shape[1]
    if m % 16 != 0 or n % 16 != 0 or k % 16 != 0:
        raise ValueError(f"{name}: M={m}, N={n} and K={k} must be multiples of 16")
    e = 1
    if offs is not None:
        offs = _offs_arg(name, offs, dev)
        e = offs.numel()
    if g_inv.dtype != torch.float32 or x_inv.dtype != torch.float32 or g_inv.numel() != e * n or x_inv.numel() != e * k:
        raise RuntimeError(f"{name}: g_inv and x_inv must be float32 [E={e}, N] and [E={e}, K], got {g_inv.dtype} {tuple(g_inv.shape)} and "
                           f"{x_inv.dtype} {tuple(x_inv.shape)}")
    g, x, g_inv, x_inv = g.contiguous(), x.contiguous(), g_inv.contiguous(), x_inv.contiguous()
    out = torch.empty((e, n, k), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_grouped_mm_wgrad(_ptr(g), _ptr(g_inv), _ptr(x), _ptr(x_inv), _ptr(offs), _ptr(out), m, n, k, e, _stream()))
    return out


def int8_quantize_rowwise_asym(x: torch.Tensor):
    """Int8Tensor.from_hp(x, PerRow(), mapping_type=ASYMMETRIC) (int8_tensor.py:191-236): bf16 [M, K] ->
    (qdata int8 [M, K], scale fp32 [M, 1], zero_point int8 [M, 1])."""
    dev = _require_gpu("int8_quantize_rowwise_asym", x)
    x = _as_rows("int8_quantize_rowwise_asym", x, torch.bfloat16)
    m, k = x.shape
    q = torch.empty((m, k), dtype=torch.int8, device=dev)
    s = torch.empty((m, 1), dtype=torch.float32, device=dev)
    zp = torch.empty((m, 1), dtype=torch.int8, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_int8_quantize_rowwise_asym(_ptr(x), _ptr(q), _ptr(s), _ptr(zp), m, k, _stream()))
    return q, s, zp


def _int8_quantize_static(name, x, scale, zero_point, pre=None):
    """The cast of x or, with `pre`, of x * pre under the given scale / zero-point."""
    dev = _require_gpu(name, x, pre, scale, zero_point)
    x, pre = _int8_rows_and_pre(name, x, pre)
    m, k = x.shape
    scale = scale.reshape(-1).to(torch.float32).contiguous()
    if scale.numel() not in (1, m):
        raise RuntimeError(f"{name}: scale must have 1 or M = {m} elements, got {scale.numel()}")
    if zero_point is not None:
        zero_point = zero_point.reshape(-1).to(torch.int8).contiguous()
        if zero_point.numel() != scale.numel():
            raise RuntimeError(f"{name}: zero_point must have the shape of scale")
    q = torch.empty((m, k), dtype=torch.int8, device=dev)
    per_row = int(scale.numel() == m and m > 1)
    with _on(dev):
        if pre is None:
            _lib.check(_lib.lib().ao_int8_quantize_static(_ptr(x), _ptr(scale), _ptr(zero_point), per_row, _ptr(q), m, k, _stream()))
        else:
            _lib.check(_lib.lib().ao_int8_quantize_static_prescaled(_ptr(x), _ptr(pre), _ptr(scale), _ptr(zero_point), per_row, _ptr(q), m, k,
                                                                    _stream()))
    return q


def int8_quantize_static(x: torch.Tensor, scale: torch.Tensor, zero_point: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Int8Tensor.from_hp(x, ..., scale=scale, zero_point=zero_point) (static quantization, int8_tensor.py:212-231): bf16 [M, K] with an fp32
    scale of 1 or M elements (and an int8 zero-point of the same shape, or None) -> qdata int8 [M, K]."""
    return _int8_quantize_static("int8_quantize_static", x, scale, zero_point)


def _int8_linear_static(xq, m, wq, w_scale, act_scale, act_zero_point, w_row_sums, bias):
    """The GEMM + epilogue behind a statically cast activation xq (zero-point-corrected when one is given)."""
    xs = act_scale.reshape(-1).to(torch.float32)
    xs = xs.expand(m) if xs.numel() == 1 else xs
    if act_zero_point is None:
        return int8_scaled_mm(xq, xs, wq, w_scale, bias)
    zp = act_zero_point.reshape(-1)
    zp = zp.expand(m) if zp.numel() == 1 else zp
    if w_row_sums is None:
        w_row_sums = int8_row_sums(wq)
    return int8_scale_epilogue_asym(int_mm(xq, wq.t()), xs, zp, w_row_sums, w_scale, bias)


def int8_linear_static(x2, wq, w_scale, act_scale, act_zero_point=None, w_row_sums=None, bias=None):
    """The Int8Tensor F.linear with STATIC activation qparams (Int8StaticActivationInt8WeightConfig): cast with the given scale /
    zero-point, then the dynamic path's GEMM + epilogue (zero-point-corrected when one is given)."""
    m = x2.shape[0]
    return _int8_linear_static(int8_quantize_static(x2, act_scale, act_zero_point), m, wq, w_scale, act_scale, act_zero_point, w_row_sums, bias)


def int8_row_sums(wq: torch.Tensor) -> torch.Tensor:
    """rowsum of an int8 [N, K] weight as int32 [N]: the zero-point correction's `weight_tensor.qdata.sum(dim=-1)` (int8_tensor.py:326)."""
    dev = _require_gpu("int8_row_sums", wq)
    wq = _as_rows("int8_row_sums", wq, torch.int8)
    n, k = wq.shape
    out = torch.empty((n,), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_int8_row_sums(_ptr(wq), _ptr(out), n, k, _stream()))
    return out


def int8_scale_epilogue_asym(acc, x_scale, x_zero_point, w_row_sums, w_scale, bias=None):
    """bf16(bf16(bf16(acc * sx[m]) - bf16((zp[m] * sx[m]) * wsum[n])) * sw[n] (+ bias)) over int32 accumulators
    (int8_tensor.py:305-346)."""
    name = "int8_scale_epilogue_asym"
    dev = _require_gpu(name, acc, x_scale, x_zero_point, w_row_sums, w_scale, bias)
    if acc.dtype != torch.int32 or acc.dim() != 2:
        raise RuntimeError(f"{name}: expected a 2-D int32 accumulator, got {acc.dim()}-D {acc.dtype}")
    acc = acc.contiguous()
    m, n = acc.shape
    x_scale = x_scale.reshape(-1).to(torch.float32).contiguous()
    x_zero_point = x_zero_point.reshape(-1).to(torch.int8).contiguous()
    w_scale = w_scale.reshape(-1).to(torch.float32).contiguous()
    w_row_sums = w_row_sums.reshape(-1).to(torch.int32).contiguous()
    if x_scale.numel() != m or x_zero_point.numel() != m or w_scale.numel() != n or w_row_sums.numel() != n:
        raise RuntimeError(f"{name}: x_scale / x_zero_point must have M = {m} entries, w_scale / w_row_sums N = {n}")
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
        if bias.numel() != n:
            raise RuntimeError(f"{name}: bias must have N elements")
    y = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_int8_scale_epilogue_asym(_ptr(acc), _ptr(x_scale), _ptr(x_zero_point), _ptr(w_row_sums), _ptr(w_scale),
                                                          _ptr(bias), _ptr(y), m, n, _stream()))
    return y


def int8_linear_asym(x2, wq, w_scale, w_row_sums, bias=None):
    """The Int8Tensor F.linear with ASYMMETRIC per-row activation quantization (int8_tensor.py:266-359): cast, int32 GEMM,
    zero-point-corrected scale epilogue (three launches; the symmetric default keeps the fused epilogue)."""
    xq, xs, zp = int8_quantize_rowwise_asym(x2)
    return int8_scale_epilogue_asym(int_mm(xq, wq.t()), xs, zp, w_row_sums, w_scale, bias)


def int8_linear_tensorwise(x2, wq, w_scale, bias=None):
    """The Int8Tensor F.linear with a PerTensor activation (int8_tensor.py:266-359): one amax over the whole activation, the
    fused two-rounding epilogue with that scalar broadcast over the rows.  `w_scale` fp32 [N] (a PerTensor weight scale already
    broadcast)."""
    xq, xs = int8_quantize_tensorwise(x2)
    return int8_scaled_mm(xq, xs.reshape(-1).expand(x2.shape[0]), wq, w_scale, bias)


def fp8_linear_tensorwise(x2, wq, w_scale, bias=None):
    """The Float8Tensor F.linear with PerTensor scales on both operands (tensorwise aten::_scaled_mm, float8/inference.py:68-123):
    `w_scale` is the weight's [1, 1] scale."""
    xq, xs = fp8_quantize_tensorwise(x2)
    n = wq.shape[0]
    return fp8_scaled_mm(xq, wq.t(), xs.reshape(-1).expand(x2.shape[0]), w_scale.reshape(-1).expand(n), bias)


def fp8_linear_clamped(x2, wq, w_scale, bias=None, lb: float = -1.0, ub: float = -1.0, tensorwise: bool = False):
    """The Float8Tensor F.linear with activation-value bounds (Float8DynamicActivationFloat8WeightConfig(activation_value_lb / _ub) ->
    hp_value_lb / hp_value_ub of _choose_scale_float8, quant_primitives.py:2203-2204): the amax (per row, or over the whole
    activation) is clamped to [lb, ub] before the scale is taken from it; values beyond ub saturate at +-448 in the cast.
    A negative bound means "not set" (the dispatcher schema has no optional floats)."""
    amax = rowwise_amax(x2)
    if tensorwise:
        amax = amax.amax().expand(x2.shape[0])
    amax = amax.clamp(min=lb if lb >= 0 else None, max=ub if ub >= 0 else None)
    amax = amax.to(torch.bfloat16).to(torch.float32)  # torch.clamp on the bf16 amax rounds the bound to bf16
    xq, xs = fp8_quantize_rowwise_amax(x2, amax)
    n = wq.shape[0]
    sb = w_scale.reshape(-1).expand(n) if w_scale.numel() == 1 else w_scale.t()
    return fp8_scaled_mm(xq, wq.t(), xs, sb, bias)


# ---------------------------------------------------------------------------
# MXFP8
# ---------------------------------------------------------------------------
MX_SCALE_MODES = {"floor": 0, "rceil": 1}


def mxfp8_quantize(x: torch.Tensor, scaling_mode: str = "rceil"):
    """Rowwise (1x32) MXFP8 cast: torchao::mxfp8_quantize(rowwise=True) /
    to_mx(x, float8_e4m3fn, 32, mode) (prototype/mx_formats/mx_tensor.py:228-409).
    x bf16 [..., C] -> (data float8_e4m3fn [..., C], scale float8_e8m0fnu [..., C/32])."""
    dev = _require_gpu("mxfp8_quantize", x)
    if x.dtype != torch.bfloat16:
        raise RuntimeError(f"mxfp8_quantize: expected bfloat16, got {x.dtype}")
    if not x.is_contiguous():
        raise RuntimeError("mxfp8_quantize: expected a contiguous tensor")  # to_mx asserts the same
    mode = MX_SCALE_MODES.get(str(getattr(scaling_mode, "value", scaling_mode)).lower())
    if mode is None:
        raise RuntimeError(f"mxfp8_quantize: unsupported scaling mode {scaling_mode!r} (floor | rceil)")
    c = x.shape[-1]
    if c % 32 != 0:
        raise RuntimeError(f"mxfp8_quantize: the last dimension of shape {tuple(x.shape)} must be divisible by 32")
    r = x.numel() // c
    q = torch.empty(x.shape, dtype=torch.uint8, device=dev)
    s = torch.empty((*x.shape[:-1], c // 32), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_mxfp8_quantize_rowwise(_ptr(x), _ptr(q), _ptr(s), r, c, mode, _stream()))
    return q.view(torch.float8_e4m3fn), s.view(torch.float8_e8m0fnu)


def fp8_grouped_mm(a, scale_a, b, scale_b, offs):
    """Float8Tensor's aten::_grouped_mm, rowwise scales (float8_tensor.py:1085-1122).  a e4m3 [M, K]; scale_a fp32 [M(,1)];
    b e4m3 [E, N, K]; scale_b fp32 [E, N(,1)]; offs int32 [E] -> bf16 [M, N] (rows past offs[-1] are zero)."""
    dev = _require_gpu("fp8_grouped_mm", a, scale_a, b, scale_b, offs)
    a = _fp8_bytes("fp8_grouped_mm", a).contiguous()
    b = _fp8_bytes("fp8_grouped_mm", b).contiguous()
    if a.dim() != 2 or b.dim() != 3 or a.shape[1] != b.shape[2]:
        raise RuntimeError(f"fp8_grouped_mm: shapes {tuple(a.shape)} and {tuple(b.shape)} are not compatible")
    m, k = a.shape
    e, n, _ = b.shape
    scale_a = scale_a.reshape(-1).to(torch.float32).contiguous()
    scale_b = scale_b.reshape(-1).to(torch.float32).contiguous()
    if scale_a.numel() != m or scale_b.numel() != e * n:
        raise RuntimeError("fp8_grouped_mm: scales must be rowwise ([M] and [E, N])")
    if offs.dtype != torch.int32 or offs.numel() != e:
        raise RuntimeError("fp8_grouped_mm: offs must be int32 [E]")
    out = torch.zeros((m, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_grouped_mm(_ptr(a), _ptr(scale_a), _ptr(b), _ptr(scale_b), _ptr(offs.contiguous()), _ptr(out), m, n, k, e,
                                                _stream()))
    return out


def mxfp8_quantize_colwise(x: torch.Tensor, scaling_mode: str = "rceil"):
    """Colwise (32x1) MXFP8 cast: torchao::mxfp8_quantize(colwise=True) == to_mx(x.t()).t()
    (csrc/cuda/mx_kernels/mxfp8_extension.cpp:160-175).  x bf16 [R, C] -> (data float8_e4m3fn {R, C} with strides {1, R},
    scale float8_e8m0fnu {C, R/32} with strides {1, C})."""
    dev = _require_gpu("mxfp8_quantize_colwise", x)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError("mxfp8_quantize_colwise: expected a contiguous 2-D bfloat16 tensor")
    mode = MX_SCALE_MODES.get(str(getattr(scaling_mode, "value", scaling_mode)).lower())
    if mode is None:
        raise RuntimeError(f"mxfp8_quantize_colwise: unsupported scaling mode {scaling_mode!r} (floor | rceil)")
    r, c = x.shape
    if r % 32 != 0 or c % 32 != 0:
        raise RuntimeError(f"mxfp8_quantize_colwise: shape {tuple(x.shape)} must be multiples of 32 in both dimensions")
    qt = torch.empty((c, r), dtype=torch.uint8, device=dev)
    st = torch.empty((r // 32, c), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_mxfp8_quantize_colwise(_ptr(x), _ptr(qt), _ptr(st), r, c, mode, _stream()))
    return qt.view(torch.float8_e4m3fn).t(), st.view(torch.float8_e8m0fnu).t()


def mxfp8_quantize_rowcol(x: torch.Tensor, scaling_mode: str = "rceil"):
    """Both casts of torchao::mxfp8_quantize(rowwise=True, colwise=True) in ONE launch that reads x once: x bf16 [R, C] ->
    (q, s, q_t_view, s_t_view) with (q, s) the bytes of mxfp8_quantize(x) and (q_t_view, s_t_view) the bytes and the strided views of
    mxfp8_quantize_colwise(x) ({R, C} strides {1, R}; {C, R/32} strides {1, C})."""
    dev = _require_gpu("mxfp8_quantize_rowcol", x)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError("mxfp8_quantize_rowcol: expected a contiguous 2-D bfloat16 tensor")
    mode = MX_SCALE_MODES.get(str(getattr(scaling_mode, "value", scaling_mode)).lower())
    if mode is None:
        raise RuntimeError(f"mxfp8_quantize_rowcol: unsupported scaling mode {scaling_mode!r} (floor | rceil)")
    r, c = x.shape
    if r % 32 != 0 or c % 32 != 0 or c == 0:
        raise RuntimeError(f"mxfp8_quantize_rowcol: shape {tuple(x.shape)} must be multiples of 32 in both dimensions")
    q = torch.empty((r, c), dtype=torch.uint8, device=dev)
    s = torch.empty((r, c // 32), dtype=torch.uint8, device=dev)
    qt = torch.empty((c, r), dtype=torch.uint8, device=dev)
    st = torch.empty((r // 32, c), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_mxfp8_quantize_rowcol(_ptr(x), _ptr(q), _ptr(s), _ptr(qt), _ptr(st), r, c, mode, _stream()))
    return (q.view(torch.float8_e4m3fn), s.view(torch.float8_e8m0fnu), qt.view(torch.float8_e4m3fn).t(), st.view(torch.float8_e8m0fnu).t())


def mxfp8_quantize_3d(x: torch.Tensor, block_size: int = 32, scale_block_dim1: int = 32, scale_block_dim2: int = 1,
                      scaling_mode: str = "rceil"):
    """mxfp8_quantize_cuda_3d with logical (un-blocked) scales (prototype/moe_training/kernels/mxfp8/quant.py:1413-1440): x bf16
    [E, N, K] -> (data float8_e4m3fn {E, N, K} column-major per expert, i.e. strides {N K, 1, N}; scale float8_e8m0fnu
    {E, K, N/32} with strides {N/32 * K, 1, K}): one scale per 32 values of the MIDDLE dimension.  Only the (32, 1) scale block."""
    dev = _require_gpu("mxfp8_quantize_3d", x)
    if x.dtype != torch.bfloat16 or x.dim() != 3 or not x.is_contiguous():
        raise RuntimeError("mxfp8_quantize_3d: expected a contiguous 3-D bfloat16 tensor")
    if block_size != 32 or (scale_block_dim1, scale_block_dim2) != (32, 1):
        raise NotImplementedError("mxfp8_quantize_3d on MI355X implements block_size 32 with (scale_block_dim1, scale_block_dim2) = (32, 1)")
    mode = MX_SCALE_MODES.get(str(getattr(scaling_mode, "value", scaling_mode)).lower())
    if mode is None:
        raise RuntimeError(f"mxfp8_quantize_3d: unsupported scaling mode {scaling_mode!r} (floor | rceil)")
    e, r, c = x.shape
    if r % 32 != 0 or c % 32 != 0:
        raise RuntimeError(f"mxfp8_quantize_3d: shape {tuple(x.shape)}: N and K must be multiples of 32")
    qt = torch.empty((e, c, r), dtype=torch.uint8, device=dev)
    st = torch.empty((e, r // 32, c), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_mxfp8_quantize_colwise_3d(_ptr(x), _ptr(qt), _ptr(st), e, r, c, mode, _stream()))
    return qt.view(torch.float8_e4m3fn).transpose(-2, -1), st.view(torch.float8_e8m0fnu).transpose(-2, -1)


def mxfp8_grouped_mm(a, a_scale, b, b_scale, offs):
    """aten::_scaled_grouped_mm for MXFP8 (mxfp8_grouped_mm.py:541), numerics of the
    emulated path (:959-1023).  a e4m3 [M, K]; a_scale e8m0 [M, K/32]; b e4m3
    [E, N, K]; b_scale e8m0 [E, N, K/32]; offs int32 [E] -> bf16 [M, N]."""
    dev = _require_gpu("mxfp8_grouped_mm", a, a_scale, b, b_scale, offs)
    a = _fp8_bytes("mxfp8_grouped_mm", a).contiguous()
    b = _fp8_bytes("mxfp8_grouped_mm", b).contiguous()
    a_scale = a_scale.view(torch.uint8).contiguous()
    b_scale = b_scale.view(torch.uint8).contiguous()
    if a.dim() != 2 or b.dim() != 3 or a.shape[1] != b.shape[2]:
        raise RuntimeError(f"mxfp8_grouped_mm: A must be [M, K] and B [E, N, K], got {tuple(a.shape)} {tuple(b.shape)}")
    m, k = a.shape
    e, n, _ = b.shape
    if tuple(a_scale.shape) != (m, k // 32) or tuple(b_scale.shape) != (e, n, k // 32):
        raise RuntimeError("mxfp8_grouped_mm: scales must be [M, K/32] and [E, N, K/32]")
    if offs.dtype != torch.int32 or offs.numel() != e:
        raise RuntimeError("mxfp8_grouped_mm: offs must be int32 [E]")
    out = torch.zeros((m, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(
            _lib.lib().ao_mxfp8_grouped_mm(
                _ptr(a), _ptr(a_scale), _ptr(b), _ptr(b_scale), _ptr(offs.contiguous()), _ptr(out), m, n, k, e, _stream()
            )
        )
    return out


def _colwise_rows(name, what, t, rows, cols):
    """The contiguous uint8 [rows, cols] tensor behind a colwise cast's output: either that tensor itself or the {cols, rows} view with
    strides {1, cols} that mxfp8_quantize_colwise returns."""
    if t.dim() == 2 and tuple(t.shape) == (cols, rows) and t.t().is_contiguous():
        return t.t()
    if t.dim() == 2 and tuple(t.shape) == (rows, cols) and t.is_contiguous():
        return t
    raise RuntimeError(f"{name}: {what} must be the contiguous [{rows}, {cols}] tensor or its transposed view (what mxfp8_quantize_colwise "
                       f"returns), got shape {tuple(t.shape)} strides {tuple(t.stride())}")


def mxfp8_grouped_mm_wgrad(g_t, g_scale, x_t, x_scale, offs, N: int, K: int):
    """The weight gradient of the MXFP8 grouped mm (mxfp8_grouped_mm.py:712-796, numerics of the emulated 2d-2d path :1026-1057), on the
    colwise (32 x 1) casts of grad_out [M, N] and x [M, K]: g_t e4m3 [N, M], g_scale e8m0 [M/32, N], x_t e4m3 [K, M], x_scale e8m0
    [M/32, K] -- or the strided views of these that mxfp8_quantize_colwise returns ({M, N} / {N, M/32} / {M, K} / {K, M/32}); offs int32
    [E] -> bf16 [E, N, K] with out[e] = dq(g)[rows of e]^T @ dq(x)[rows of e]; an empty group gives zeros.  Any offsets."""
    name = "mxfp8_grouped_mm_wgrad"
    dev = _require_gpu(name, g_t, g_scale, x_t, x_scale, offs)
    n, k = int(N), int(K)
    if n <= 0 or k <= 0 or g_t.numel() % n != 0:
        raise RuntimeError(f"{name}: g_t with {g_t.numel()} elements does not hold [N={n}, M] codes")
    m = g_t.numel() // n
    if m % 32 != 0:
        raise RuntimeError(f"{name}: M_total={m} must be a multiple of 32 (one scale per 32 tokens)")
    if g_scale.dtype not in (torch.uint8, torch.float8_e8m0fnu) or x_scale.dtype not in (torch.uint8, torch.float8_e8m0fnu):
        raise RuntimeError(f"{name}: expected float8_e8m0fnu scales, got {g_scale.dtype} and {x_scale.dtype}")
    g = _colwise_rows(name, "g_t", _fp8_bytes(name, g_t), n, m)
    x = _colwise_rows(name, "x_t", _fp8_bytes(name, x_t), k, m)
    gs = _colwise_rows(name, "g_scale", g_scale.view(torch.uint8), m // 32, n)
    xs = _colwise_rows(name, "x_scale", x_scale.view(torch.uint8), m // 32, k)
    if offs.dtype != torch.int32 or offs.dim() != 1 or offs.numel() < 1:
        raise RuntimeError(f"{name}: offs must be int32 [E]")
    e = offs.numel()
    out = torch.empty((e, n, k), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_mxfp8_grouped_mm_wgrad(_ptr(g), _ptr(gs), _ptr(x), _ptr(xs), _ptr(offs.contiguous()), _ptr(out), m, n, k, e,
                                                        _stream()))
    return out


def mxfp8_mm_wgrad(g_t, g_scale, x_t, x_scale, N: int, K: int):
    """The weight gradient of a dense MXFP8 linear (mxfp8_linear.py:208-255) on the colwise (32 x 1) casts of grad_out [M, N] and x [M, K],
    in the layouts mxfp8_grouped_mm_wgrad takes -> bf16 [N, K] = dq(g)^T @ dq(x): the grouped kernel over one group of every token, no offs
    tensor.  The bits of mxfp8_grouped_mm_wgrad(..., offs=[M])[0]; M = 0 gives zeros."""
    name = "mxfp8_mm_wgrad"
    dev = _require_gpu(name, g_t, g_scale, x_t, x_scale)
    n, k = int(N), int(K)
    if n <= 0 or k <= 0 or g_t.numel() % n != 0:
        raise RuntimeError(f"{name}: g_t with {g_t.numel()} elements does not hold [N={n}, M] codes")
    m = g_t.numel() // n
    if m % 32 != 0:
        raise RuntimeError(f"{name}: M={m} must be a multiple of 32 (one scale per 32 tokens)")
    if g_scale.dtype not in (torch.uint8, torch.float8_e8m0fnu) or x_scale.dtype not in (torch.uint8, torch.float8_e8m0fnu):
        raise RuntimeError(f"{name}: expected float8_e8m0fnu scales, got {g_scale.dtype} and {x_scale.dtype}")
    g = _colwise_rows(name, "g_t", _fp8_bytes(name, g_t), n, m)
    x = _colwise_rows(name, "x_t", _fp8_bytes(name, x_t), k, m)
    gs = _colwise_rows(name, "g_scale", g_scale.view(torch.uint8), m // 32, n)
    xs = _colwise_rows(name, "x_scale", x_scale.view(torch.uint8), m // 32, k)
    out = torch.empty((n, k), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_mxfp8_mm_wgrad(_ptr(g), _ptr(gs), _ptr(x), _ptr(xs), _ptr(out), m, n, k, _stream()))
    return out


def _mx_mode(scaling_mode) -> int:
    mode = MX_SCALE_MODES.get(str(getattr(scaling_mode, "value", scaling_mode)).lower())
    if mode is None:
        raise RuntimeError(f"unsupported MX scaling mode {scaling_mode!r} (floor | rceil)")
    return mode


def mxfp8_grouped_mm_dyn_fits(m, n, k, e) -> bool:
    """Whether mxfp8_grouped_mm_dyn takes the shape with aligned operands (host logic: decode-size groups, K % 512 == 0)."""
    return bool(_lib.lib().ao_mxfp8_grouped_mm_dyn_fits(int(m), int(n), int(k), int(e)))


def mxfp8_grouped_mm_fuses(a, *b_scales) -> bool:
    """Whether mxfp8_grouped_mm_dyn (one weight scale) / mxfp8_grouped_mm_pair (two) takes the BF16 activations `a` in ONE launch: the
    route (ao_grouped8_route) for these tensors as they reach the C entry point, after .contiguous().  Else cast + mxfp8_grouped_mm."""
    e, n, _ = b_scales[0].shape
    aligned = all(t.contiguous().data_ptr() % 16 == 0 for t in (a, *b_scales))
    out = (ctypes.c_int32 * 10)()
    _lib.check(_lib.lib().ao_grouped8_route(2 if len(b_scales) == 1 else 3, a.shape[0], n, a.shape[1], e, int(aligned), out, 10))
    return out[0] != 0


def mxfp8_grouped_mm_dyn(a, b, b_scale, offs, scaling_mode="rceil"):
    """to_mx(a) + the MXFP8 grouped mm in ONE launch (mxfp8_grouped_mm.py:330-371): a bf16 [M, K]; b e4m3 [E, N, K];
    b_scale e8m0 [E, N, K/32]; offs int32 [E] -> bf16 [M, N], bit-identical to mxfp8_quantize(a) followed by mxfp8_grouped_mm.  Rows past
    offs[-1] are left unwritten (torch._scaled_grouped_mm's contract; mxfp8_grouped_mm zero-fills them)."""
    dev = _require_gpu("mxfp8_grouped_mm_dyn", a, b, b_scale, offs)
    if a.dtype != torch.bfloat16 or a.dim() != 2:
        raise RuntimeError(f"mxfp8_grouped_mm_dyn: a must be a 2-D bfloat16 tensor, got {a.dtype} {tuple(a.shape)}")
    a = a.contiguous()
    b = _fp8_bytes("mxfp8_grouped_mm_dyn", b).contiguous()
    b_scale = b_scale.view(torch.uint8).contiguous()
    if b.dim() != 3 or a.shape[1] != b.shape[2]:
        raise RuntimeError(f"mxfp8_grouped_mm_dyn: A must be [M, K] and B [E, N, K], got {tuple(a.shape)} {tuple(b.shape)}")
    m, k = a.shape
    e, n, _ = b.shape
    if tuple(b_scale.shape) != (e, n, k // 32):
        raise RuntimeError("mxfp8_grouped_mm_dyn: b_scale must be [E, N, K/32]")
    if offs.dtype != torch.int32 or offs.numel() != e:
        raise RuntimeError("mxfp8_grouped_mm_dyn: offs must be int32 [E]")
    out = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_mxfp8_grouped_mm_dyn(_ptr(a), _ptr(b), _ptr(b_scale), _ptr(offs.contiguous()), _ptr(out), m, n, k, e,
                                                      _mx_mode(scaling_mode), _stream()))
    return out


def mxfp8_grouped_mm_pair_fits(m, n, k, e) -> bool:
    """Whether the pair forms take the shape (host logic: the mxfp8_grouped_mm_dyn conditions with twice the tiles)."""
    return bool(_lib.lib().ao_mxfp8_grouped_mm_pair_fits(int(m), int(n), int(k), int(e)))


def mxfp8_grouped_mm_pair(a, b1, b1_scale, b3, b3_scale, offs, scaling_mode="rceil", a_scale=None):
    """x @ w1 and x @ w3 of an MoE layer in ONE launch: two expert-weight tensors of one shape [E, N, K] (e4m3 + E8M0 [E, N, K/32]) against
    the same activations.  a bf16 [M, K] (the 1 x 32 cast fused into the kernel, as mxfp8_grouped_mm_dyn) or, with a_scale, its e4m3 codes.
    -> (y1, y3) bf16 [M, N]: the two single products' values -- bit for bit where the stream-K shares cut the tiles at the same k steps as the
    single launches do, else up to the fp32 summation order of a cut tile's pieces (single elements one bf16 ulp apart; reproducible from
    launch to launch).  Rows past offs[-1] are left unwritten."""
    dev = _require_gpu("mxfp8_grouped_mm_pair", a, b1, b1_scale, b3, b3_scale, offs)
    b1 = _fp8_bytes("mxfp8_grouped_mm_pair", b1).contiguous()
    b3 = _fp8_bytes("mxfp8_grouped_mm_pair", b3).contiguous()
    b1_scale, b3_scale = b1_scale.view(torch.uint8).contiguous(), b3_scale.view(torch.uint8).contiguous()
    if a.dim() != 2 or b1.dim() != 3 or b1.shape != b3.shape or a.shape[1] != b1.shape[2]:
        raise RuntimeError(f"mxfp8_grouped_mm_pair: A must be [M, K] and both B [E, N, K], got {tuple(a.shape)} {tuple(b1.shape)} {tuple(b3.shape)}")
    m, k = a.shape
    e, n, _ = b1.shape
    if tuple(b1_scale.shape) != (e, n, k // 32) or tuple(b3_scale.shape) != (e, n, k // 32):
        raise RuntimeError("mxfp8_grouped_mm_pair: weight scales must be [E, N, K/32]")
    if offs.dtype != torch.int32 or offs.numel() != e:
        raise RuntimeError("mxfp8_grouped_mm_pair: offs must be int32 [E]")
    y1 = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    y3 = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        if a_scale is None:
            if a.dtype != torch.bfloat16:
                raise RuntimeError(f"mxfp8_grouped_mm_pair: a must be bfloat16 (or e4m3 codes with a_scale), got {a.dtype}")
            _lib.check(_lib.lib().ao_mxfp8_grouped_mm_dyn_pair(_ptr(a.contiguous()), _ptr(b1), _ptr(b1_scale), _ptr(b3), _ptr(b3_scale), _ptr(offs.contiguous()),
                                                               _ptr(y1), _ptr(y3), m, n, k, e, _mx_mode(scaling_mode), _stream()))
        else:
            aq = _fp8_bytes("mxfp8_grouped_mm_pair", a).contiguous()
            asc = a_scale.view(torch.uint8).contiguous()
            if tuple(asc.shape) != (m, k // 32):
                raise RuntimeError("mxfp8_grouped_mm_pair: a_scale must be [M, K/32]")
            _lib.check(_lib.lib().ao_mxfp8_grouped_mm_pair(_ptr(aq), _ptr(asc), _ptr(b1), _ptr(b1_scale), _ptr(b3), _ptr(b3_scale), _ptr(offs.contiguous()),
                                                           _ptr(y1), _ptr(y3), m, n, k, e, _stream()))
    return y1, y3


def _check_token_groups(name, inputs, offsets):
    if inputs.dim() != 2:
        raise AssertionError("input activations must be 2d")
    if inputs.dtype not in (torch.float32, torch.bfloat16):
        raise AssertionError("inputs must be float32 or bfloat16")
    if offsets.dtype != torch.int32:
        raise AssertionError("offsets must be int32")
    if offsets.dim() != 1 or offsets.numel() == 0:
        raise RuntimeError(f"{name}: offsets must be a non-empty 1-d tensor of group end offsets")


def fused_pad_token_groups(inputs, offsets, alignment_size=32):
    """torchao::fused_pad_token_groups (kernels/mxfp8/quant.py:1244-1283; semantics torch_pad_token_groups,
    quant.py:368-430): every token group is moved to a start that is a multiple of `alignment_size` inside a
    zero-filled buffer of the reference's upper-bound size (no host sync).  Returns (padded_tokens,
    padded_group_start_offsets, padded_group_end_offsets)."""
    dev = _require_gpu("fused_pad_token_groups", inputs, offsets)
    _check_token_groups("fused_pad_token_groups", inputs, offsets)
    inputs = inputs.contiguous()
    offsets = offsets.contiguous()
    tokens, dim = inputs.shape
    groups = offsets.numel()
    if alignment_size <= 0:
        raise ValueError(f"fused_pad_token_groups: alignment_size must be positive, got {alignment_size}")
    rows = _lib.lib().ao_moe_padded_rows(tokens, groups, alignment_size)
    padded = torch.empty((rows, dim), dtype=inputs.dtype, device=dev)  # the kernel writes every row
    starts = torch.empty(groups, dtype=torch.int32, device=dev)
    ends = torch.empty(groups, dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(
            _lib.lib().ao_moe_pad_token_groups(
                _ptr(inputs), _ptr(offsets), _ptr(padded), _ptr(starts), _ptr(ends), tokens, dim, inputs.element_size(), groups,
                alignment_size, _stream()
            )
        )
    return padded, starts, ends


def _scale_bytes(name, scales):
    if scales.dim() != 2:
        raise AssertionError("scales_tensor must be 2D")
    if scales.dtype not in (torch.uint8, torch.float8_e8m0fnu):
        raise AssertionError("scales_tensor must be uint8 or float8_e8m0fnu")
    return scales.contiguous()


def mx_block_rearrange_2d_M_groups(scales_tensor, input_offsets, chunks_per_tb=4):
    """torchao::mx_block_rearrange_2d_M_groups (kernels/mxfp8/quant.py:969-973, 1183-1225; semantics torch_to_blocked_2d_M_groups,
    quant.py:136-196): E8M0 scales [rows, cols] of token groups ending at `input_offsets` -> the reference's 128 x 4 blocked layout, every
    group padded to 128-row blocks, in a [rows + 128 groups, 4 ceil(cols / 4)] tensor (zero elsewhere).  `chunks_per_tb` is the
    reference's launch-shape knob: validated, no meaning here."""
    dev = _require_gpu("mx_block_rearrange_2d_M_groups", scales_tensor, input_offsets)
    s = _scale_bytes("mx_block_rearrange_2d_M_groups", scales_tensor)
    if input_offsets.dtype != torch.int32:
        raise AssertionError("input_offsets must be int32")
    if input_offsets.dim() != 1 or input_offsets.numel() == 0:
        raise RuntimeError("mx_block_rearrange_2d_M_groups: input_offsets must be a non-empty 1-d tensor of group end offsets")
    if chunks_per_tb not in (1, 4, 8, 16):
        raise AssertionError("chunks_per_tb must be 1, 4, 8, or 16")
    rows, cols = s.shape
    groups = input_offsets.numel()
    out = torch.empty((_lib.lib().ao_mx_blocked_rows(rows, groups), (cols + 3) // 4 * 4), dtype=s.dtype, device=dev)  # every byte is written
    with _on(dev):
        _lib.check(_lib.lib().ao_mx_block_rearrange_2d_m_groups(_ptr(s), _ptr(input_offsets.contiguous()), _ptr(out), rows, cols, groups, _stream()))
    return out


def mx_to_blocked(scales_tensor):
    """to_blocked (prototype/mx_formats/utils.py:31-72): E8M0 scales [H, W] -> flat 32 ceil(H / 128) x 16 ceil(W / 4) bytes in the 128 x 4
    blocked layout."""
    dev = _require_gpu("mx_to_blocked", scales_tensor)
    s = _scale_bytes("mx_to_blocked", scales_tensor)
    rows, cols = s.shape
    out = torch.empty(((rows + 127) // 128 * 128) * ((cols + 3) // 4 * 4), dtype=s.dtype, device=dev)
    if out.numel():
        with _on(dev):
            _lib.check(_lib.lib().ao_mx_to_blocked(_ptr(s), _ptr(out), rows, cols, _stream()))
    return out


def fp8_int4_linear(xq, x_scale, qdata, scale_and_zero, group_size, bias=None):
    """mslk.f8i4bf16_rowwise's contract (int4_tensor.py:213-229): e4m3 activations [M, K] with per-row fp32 scales x int4 weights in the
    tinygemm tile order (offset-8 codes; scale_and_zero bf16 [K/g, N, 2]) -> bf16 [M, N]; the group scale multiplies fp32 group sums."""
    dev = _require_gpu("fp8_int4_linear", xq, x_scale, qdata, scale_and_zero)
    xq = _fp8_bytes("fp8_int4_linear", xq)
    if xq.dim() != 2 or qdata.dim() != 4 or qdata.dtype != torch.int32 or scale_and_zero.dtype != torch.bfloat16:
        raise RuntimeError("fp8_int4_linear: expected xq [M, K] e4m3, qdata int32 [N/8, K/128, 32, 4], scale_and_zero bf16 [K/g, N, 2]")
    m, k = xq.shape
    n = qdata.shape[0] * 8
    if qdata.shape[1] * 128 != k or tuple(scale_and_zero.shape) != (k // group_size, n, 2):
        raise RuntimeError(f"fp8_int4_linear: shapes do not agree: xq {tuple(xq.shape)}, qdata {tuple(qdata.shape)}, scale_and_zero {tuple(scale_and_zero.shape)}")
    xs = x_scale.reshape(-1).to(torch.float32).contiguous()
    if xs.numel() != m:
        raise RuntimeError("fp8_int4_linear: one activation scale per row expected")
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_int4_linear(_ptr(xq.contiguous()), _ptr(xs), _ptr(qdata.contiguous()), _ptr(scale_and_zero.contiguous()),
                                                 _ptr(bias) if bias is not None else None, _ptr(y), m, n, k, group_size, _stream()))
    return y


def fp8_int4_dynamic_fits(m: int, n: int, k: int) -> bool:
    """Whether the fp8-activation x int4 kernel with the activation cast fused in takes this shape (M <= 16, codes within 64 KiB of LDS)."""
    return bool(_lib.lib().ao_fp8_int4_dynamic_fits(m, n, k))


def fp8_int4_act_linear(x, qdata, scale_and_zero, group_size, bias=None, fused=None):
    """Float8DynamicActivationInt4WeightConfig's F.linear on a 2-D bf16 activation (int4_tensor.py:205-235): per-row e4m3 cast of x, then
    mslk.f8i4bf16_rowwise's contract.  One row runs cast + matmul in ONE launch (round 4: the stand-alone cast cost this path 28 %);
    everything else ao_fp8_quantize_rowwise + ao_fp8_int4_linear.  Same bits either way."""
    dev = _require_gpu("fp8_int4_act_linear", x, qdata, scale_and_zero)
    if x.dim() != 2 or x.dtype != torch.bfloat16:
        raise RuntimeError(f"fp8_int4_act_linear: x must be a 2-D bfloat16 tensor, got {tuple(x.shape)} {x.dtype}")
    m, k = x.shape
    n = qdata.shape[0] * 8
    # (round 6, tools/bench_fp8_int4.py --batch 1 .. 16, the 160 linears of a Llama-3-8B token, profiles/f3_fused_vs_cast_r06.jsonl: the
    # fused launch is 1.23 x ahead of cast + matmul at one row, level at two, and 1.17 / 1.32 / 1.72 x BEHIND at 3 / 4 / 8 rows -- every
    # workgroup casts all rows itself -- so it serves one row only)
    # `fused`: None = that rule; True = the one-launch form wherever the kernel takes the shape (tests, A/B)
    if not fp8_int4_dynamic_fits(m, n, k) or not (fused if fused is not None else m == 1):
        xq, xs = fp8_quantize_rowwise(x.contiguous())
        return fp8_int4_linear(xq, xs, qdata, scale_and_zero, group_size, bias)
    if qdata.dim() != 4 or qdata.dtype != torch.int32 or scale_and_zero.dtype != torch.bfloat16 or qdata.shape[1] * 128 != k \
            or tuple(scale_and_zero.shape) != (k // group_size, n, 2):
        raise RuntimeError(f"fp8_int4_act_linear: shapes do not agree: x {tuple(x.shape)}, qdata {tuple(qdata.shape)}, scale_and_zero {tuple(scale_and_zero.shape)}")
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    y = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_int4_dynamic_linear(_ptr(x.contiguous()), _ptr(qdata.contiguous()), _ptr(scale_and_zero.contiguous()),
                                                         _ptr(bias) if bias is not None else None, _ptr(y), m, n, k, group_size, _stream()))
    return y


def generate_permute_indices(tokens_per_expert_group, experts_per_rank, num_ranks, max_len, alignment):
    """torchao.prototype.moe_training.ep.kernels.generate_permute_indices (kernels.py:132-214): expert-major gather indices with every
    expert's group padded to `alignment` rows.  Returns (permuted_indices int32 [max_len] with -1 for padding, m_sizes int32 [E],
    m_offsets int32 [E])."""
    dev = _require_gpu("generate_permute_indices", tokens_per_expert_group)
    counts = tokens_per_expert_group.to(torch.int32).contiguous()
    if counts.numel() != experts_per_rank * num_ranks:
        raise ValueError(f"generate_permute_indices: expected {experts_per_rank * num_ranks} counts, got {counts.numel()}")
    idx = torch.empty(max_len, dtype=torch.int32, device=dev)
    start = torch.empty(counts.numel(), dtype=torch.int32, device=dev)
    m_sizes = torch.empty(experts_per_rank, dtype=torch.int32, device=dev)
    m_offsets = torch.empty(experts_per_rank, dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_moe_permute_indices(_ptr(counts), _ptr(start), _ptr(idx), _ptr(m_sizes), _ptr(m_offsets), experts_per_rank,
                                                     num_ranks, max_len, alignment, _stream()))
    return idx, m_sizes, m_offsets


def _rows_u8(t):
    """[rows, row_bytes] byte view of a 2-D tensor of any dtype"""
    t = t.contiguous()
    return t, t.shape[0], t.shape[1] * t.element_size()


def gather_rows(x, indices, num_out=None):
    """out[i] = x[indices[i]] for 0 <= indices[i] < rows(x), zeros otherwise (`vstack(x, 0)[indices]`, ep/permute.py:86-96).
    `num_out` (at most the number of indices): only the first num_out output rows."""
    if x.dim() != 2 or indices.dim() != 1 or indices.dtype != torch.int32:
        raise ValueError("gather_rows: expected a 2-D tensor and int32 1-D indices")
    n_out = indices.numel() if num_out is None else int(num_out)
    if n_out < 0 or n_out > indices.numel():  # the kernel reads one index per output row
        raise ValueError(f"gather_rows: num_out={n_out} must be in [0, {indices.numel()}], the number of indices")
    dev = _require_gpu("gather_rows", x, indices)
    x, rows, row_bytes = _rows_u8(x)
    indices = indices.contiguous()
    out = torch.empty((n_out, x.shape[1]), dtype=x.dtype, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_moe_gather_rows(_ptr(x), _ptr(indices), _ptr(out), rows, n_out, row_bytes, _stream()))
    return out


def scatter_rows(y, indices, num_rows_out):
    """out[indices[i]] = y[i] for 0 <= indices[i] < num_rows_out (`out = empty(rows + 1); out[indices] = y; out[:-1]`,
    ep/unpermute.py:36-41).  Rows no index names are left uninitialised, like the reference's."""
    dev = _require_gpu("scatter_rows", y, indices)
    if y.dim() != 2 or indices.dim() != 1 or indices.dtype != torch.int32 or indices.numel() != y.shape[0]:
        raise ValueError("scatter_rows: expected a 2-D tensor and one int32 index per row")
    y, rows, row_bytes = _rows_u8(y)
    indices = indices.contiguous()
    out = torch.empty((num_rows_out, y.shape[1]), dtype=y.dtype, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_moe_scatter_rows(_ptr(y), _ptr(indices), _ptr(out), rows, num_rows_out, row_bytes, _stream()))
    return out


def fused_unpad_token_groups(inputs, offsets, padded_group_start_offsets, num_tokens, alignment_size=32):
    """torchao::fused_unpad_token_groups (kernels/mxfp8/quant.py:1319-1363; semantics torch_unpad_token_groups,
    quant.py:433-480): gathers the `num_tokens` real rows back out of a padded buffer."""
    dev = _require_gpu("fused_unpad_token_groups", inputs, offsets, padded_group_start_offsets)
    _check_token_groups("fused_unpad_token_groups", inputs, offsets)
    if padded_group_start_offsets.dtype != torch.int32:
        raise AssertionError("padded_group_start_offsets must be int32")
    if padded_group_start_offsets.numel() != offsets.numel():
        raise RuntimeError("fused_unpad_token_groups: offsets and padded_group_start_offsets must have one entry per group")
    inputs = inputs.contiguous()
    dim = inputs.shape[1]
    out = torch.empty((num_tokens, dim), dtype=inputs.dtype, device=dev)
    with _on(dev):
        _lib.check(
            _lib.lib().ao_moe_unpad_token_groups(
                _ptr(inputs), _ptr(offsets.contiguous()), _ptr(padded_group_start_offsets.contiguous()), _ptr(out), num_tokens, dim,
                inputs.element_size(), offsets.numel(), _stream()
            )
        )
    return out


def dynamic_linear_fits(m: int, n: int, k: int) -> bool:
    """Whether the fused cast + matmul kernels take this shape (M <= 16: the cast activation must fit LDS; 16 < M <= 256: weights with
    few output tiles and K % 512 == 0)."""
    return bool(_lib.lib().ao_dyn_linear_fits(m, n, k))


def dynamic_linear_preferred(m: int, n: int, k: int) -> bool:
    """Whether the fused kernel beats cast + matmul: every workgroup (one per 16 output columns) casts the whole activation itself, so
    the redundant work grows with M while the stand-alone cast stays one ~3 us launch.  Round 6 re-measured both forms of the whole linear
    on a bf16 activation (tools/bench_dec8.py --linear --all-shapes, 8 shapes x int8 / fp8 x M = 1 .. 16, cold weights,
    profiles/dyn_vs_two_r06.jsonl): fused wins at M = 1 on every shape (qkv shard 5.0 vs 7.5 us, o 3.7 vs 6.2, gate_up 13.7 vs 15.7, down
    4096 x 14336 15.8 vs 16.9), M = 2 is level (+- 5 %), and from 3 rows on cast + matmul is 1.2 - 1.6 x ahead wherever the rule of
    rounds 2 - 5 (M x N / 16 <= 1024) still took the fused kernel (qkv shard at M = 6: 14.4 vs 9.1 us) -- the decode matmul got faster
    since (full-line ring, 8-row tiles, the LDS bound), the in-kernel cast did not.  16 < M <= 256 (mid8_kernels.hip) is reachable but was
    never preferred (profiles/mid8_sweep_r04.txt)."""
    return m == 1 and dynamic_linear_fits(m, n, k)


def int8_linear(x2: torch.Tensor, wq: torch.Tensor, w_scale: torch.Tensor, bias=None) -> torch.Tensor:
    """The Int8Tensor dynamic-activation F.linear on a 2-D bf16 activation (int8_tensor.py:266-359): decode sizes take the
    fused cast + matmul kernel, everything else ao_int8_quantize_rowwise + ao_int8_scaled_mm.  Same bits either way."""
    if dynamic_linear_preferred(x2.shape[0], wq.shape[0], x2.shape[1]):
        return int8_dynamic_linear(x2, wq, w_scale, bias)
    xq, xs = int8_quantize_rowwise(x2)
    return int8_scaled_mm(xq, xs, wq, w_scale, bias)


def fp8_linear(x2: torch.Tensor, wq: torch.Tensor, w_scale: torch.Tensor, bias=None) -> torch.Tensor:
    """The Float8Tensor rowwise dynamic-activation F.linear on a 2-D bf16 activation (float8_tensor.py:338-469)."""
    if dynamic_linear_preferred(x2.shape[0], wq.shape[0], x2.shape[1]):
        return fp8_dynamic_linear(x2, wq, w_scale, bias)
    xq, xs = fp8_quantize_rowwise(x2)
    return fp8_scaled_mm(xq, wq.t(), xs, w_scale.t(), bias)


def _dynamic_linear(name, entry, x, wq, w_scale, bias, wdtype):
    dev = _require_gpu(name, x, wq, w_scale, bias)
    if x.dim() != 2 or x.dtype != torch.bfloat16:
        raise RuntimeError(f"{name}: x must be a 2-D bfloat16 tensor, got {tuple(x.shape)} {x.dtype}")
    if wq.dim() != 2 or wq.dtype != wdtype:
        raise RuntimeError(f"{name}: weight must be a 2-D {wdtype} tensor [N, K]")
    x = x.contiguous()
    wq = wq.contiguous()
    m, k = x.shape
    n, k2 = wq.shape
    if k != k2:
        raise RuntimeError(f"{name}: K mismatch {k} vs {k2}")
    w_scale = w_scale.reshape(-1).to(torch.float32).contiguous()
    if w_scale.numel() != n:
        raise RuntimeError(f"{name}: weight scale must be per-row ([N])")
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
        if bias.numel() != n:
            raise RuntimeError(f"{name}: bias must have N elements")
    y = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(entry(_ptr(x), _ptr(wq.view(torch.uint8) if wdtype != torch.int8 else wq), _ptr(w_scale), _ptr(bias), _ptr(y), m, n, k, _stream()))
    return y


def int8_dynamic_linear(x, wq, w_scale, bias=None):
    """Int8Tensor F.linear with dynamic per-row activation quantisation in ONE launch (int8_tensor.py:176-248, 305-359): same
    bits as int8_quantize_rowwise + int8_scaled_mm.  Shapes accepted: dynamic_linear_fits(M, N, K)."""
    return _dynamic_linear("int8_dynamic_linear", _lib.lib().ao_int8_dynamic_linear, x, wq, w_scale, bias, torch.int8)


def fp8_dynamic_linear(x, wq, w_scale, bias=None):
    """Float8Tensor F.linear with dynamic per-row e4m3 activation quantisation in ONE launch (float8_tensor.py:167-253,
    float8/inference.py:104-123): same bits as fp8_quantize_rowwise + fp8_scaled_mm at these sizes."""
    return _dynamic_linear("fp8_dynamic_linear", _lib.lib().ao_fp8_dynamic_linear, x, wq, w_scale, bias, torch.float8_e4m3fn)


# ---- MX dense linears (MXFP4 / MXFP8; include/ao_mi355.h "MX dense linears") ------------------------------------
MX_FMT_E4M3 = 0  # the scaled MFMA's format codes
MX_FMT_E2M1 = 4
_MX_FMTS = {MX_FMT_E4M3, MX_FMT_E2M1}


def mx_fmt(elem_dtype) -> int:
    """torch element dtype of an MXTensor -> the C ABI's fmt code (float8_e4m3fn 0, float4_e2m1fn_x2 4)."""
    if elem_dtype == torch.float8_e4m3fn:
        return MX_FMT_E4M3
    if elem_dtype == torch.float4_e2m1fn_x2:
        return MX_FMT_E2M1
    raise NotImplementedError(f"MX linears on MI355X take float8_e4m3fn or float4_e2m1fn_x2 elements, got {elem_dtype}")


def mxfp4_quantize(x: torch.Tensor, scaling_mode: str = "rceil"):
    """Rowwise (1x32) MXFP4 cast: to_mx(x, float4_e2m1fn_x2, 32, mode) (prototype/mx_formats/mx_tensor.py:228-409).
    x bf16 [..., C] -> (data uint8 [..., C/2] packed e2m1 codes, element 2i in the low nibble; scale float8_e8m0fnu [..., C/32])."""
    dev = _require_gpu("mxfp4_quantize", x)
    if x.dtype != torch.bfloat16:
        raise RuntimeError(f"mxfp4_quantize: expected bfloat16, got {x.dtype}")
    if not x.is_contiguous():
        raise RuntimeError("mxfp4_quantize: expected a contiguous tensor")
    mode = _mx_mode(scaling_mode)
    c = x.shape[-1]
    if c % 32 != 0 or c == 0:
        raise RuntimeError(f"mxfp4_quantize: the last dimension of shape {tuple(x.shape)} must be divisible by 32")
    r = x.numel() // c
    q = torch.empty((*x.shape[:-1], c // 2), dtype=torch.uint8, device=dev)
    s = torch.empty((*x.shape[:-1], c // 32), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_mxfp4_quantize_rowwise(_ptr(x), _ptr(q), _ptr(s), r, c, mode, _stream()))
    return q, s.view(torch.float8_e8m0fnu)


def mx_quantize(x: torch.Tensor, fmt: int, scaling_mode="rceil"):
    """(codes, scales) of the 1 x 32 cast of bf16 x for fmt (MX_FMT_E4M3 / MX_FMT_E2M1)."""
    if fmt == MX_FMT_E2M1:
        return mxfp4_quantize(x, scaling_mode)
    return mxfp8_quantize(x, scaling_mode)


MX_LINEAR_KERNELS = {0: "invalid", 1: "mx_linear_stream_kernel", 2: "mx_linear_tile_kernel"}


# The queries of the two-form linear families (csrc/two_form_route.h): the C entry by name, then its integer arguments.
def _two_form_route(entry, kernels, *ints):
    out = (ctypes.c_int32 * 7)()
    _lib.check(getattr(_lib.lib(), entry)(*map(int, ints), out, 7))
    kernel, waves, mt, tile_m, tile_n, gx, gy = list(out)
    return {"kernel": kernels.get(kernel, "invalid"), "waves": waves, "m_tiles": mt, "tile_m": tile_m, "tile_n": tile_n, "grid": (gx, gy)}


def _two_form_kernel_name(entry, *ints):
    return getattr(_lib.lib(), entry)(*map(int, ints)).decode()


def _two_form_set_form(entry, form):
    _lib.check(getattr(_lib.lib(), entry)(int(form)))


def mx_linear_route(fmt: int, m: int, n: int, k: int) -> dict:
    """The route mx_mm / mx_linear launch for a shape (host logic only, ao_mx_linear_route)."""
    return _two_form_route("ao_mx_linear_route", MX_LINEAR_KERNELS, fmt, m, n, k)


def mx_linear_kernel_name(fmt: int, m: int, n: int, k: int) -> str:
    return _two_form_kernel_name("ao_mx_linear_kernel_name", fmt, m, n, k)


def mx_linear_set_form(form: int) -> None:
    """Measurement only: 0 the product route, 1 the streaming form, 2 the tiled form (calling thread)."""
    _two_form_set_form("ao_mx_linear_set_form", form)


def _mx_operands(name, fmt, b, b_scale, bias, k_from_a):
    if fmt not in _MX_FMTS:
        raise RuntimeError(f"{name}: fmt must be {MX_FMT_E4M3} (e4m3) or {MX_FMT_E2M1} (e2m1), got {fmt}")
    b = b.view(torch.uint8) if b.dtype in (torch.float8_e4m3fn, torch.float4_e2m1fn_x2) else b
    if b.dtype != torch.uint8 or b.dim() != 2:
        raise RuntimeError(f"{name}: the weight codes must be a 2-D uint8 / e4m3 tensor [N, K or K/2], got {b.dtype} {tuple(b.shape)}")
    n = b.shape[0]
    k = b.shape[1] * (2 if fmt == MX_FMT_E2M1 else 1)
    if k != k_from_a:
        raise RuntimeError(f"{name}: K of the activation ({k_from_a}) and of the weight ({k}) differ")
    b_scale = b_scale.view(torch.uint8)
    if tuple(b_scale.shape) != (n, k // 32):
        raise RuntimeError(f"{name}: the weight scales must be [N, K/32] = {(n, k // 32)}, got {tuple(b_scale.shape)}")
    if bias is not None and (bias.dtype != torch.bfloat16 or bias.numel() != n):
        raise RuntimeError(f"{name}: bias must be bfloat16 [N], got {bias.dtype} {tuple(bias.shape)}")
    return b.contiguous(), b_scale.contiguous(), (bias.contiguous() if bias is not None else None), n, k


def mx_mm(a, a_scale, b, b_scale, bias=None, fmt: int = MX_FMT_E2M1):
    """The MX GEMM on codes: a [M, K or K/2], a_scale [M, K/32], b [N, K or K/2] (the weight as stored), b_scale [N, K/32], bias bf16 [N]
    -> bf16 [M, N] = bf16(sum_k dq(a) dq(b) + bias), fp32 accumulation (ao_mx_linear)."""
    dev = _require_gpu("mx_mm", a, a_scale, b, b_scale, bias)
    a = a.view(torch.uint8) if a.dtype in (torch.float8_e4m3fn, torch.float4_e2m1fn_x2) else a
    if a.dtype != torch.uint8 or a.dim() != 2:
        raise RuntimeError(f"mx_mm: the activation codes must be a 2-D uint8 / e4m3 tensor, got {a.dtype} {tuple(a.shape)}")
    m = a.shape[0]
    ka = a.shape[1] * (2 if fmt == MX_FMT_E2M1 else 1)
    b, b_scale, bias, n, k = _mx_operands("mx_mm", fmt, b, b_scale, bias, ka)
    a_scale = a_scale.view(torch.uint8).contiguous()
    if tuple(a_scale.shape) != (m, k // 32):
        raise RuntimeError(f"mx_mm: the activation scales must be [M, K/32] = {(m, k // 32)}, got {tuple(a_scale.shape)}")
    out = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    if m == 0:
        return out
    with _on(dev):
        _lib.check(_lib.lib().ao_mx_linear(int(fmt), _ptr(a.contiguous()), _ptr(a_scale), _ptr(b), _ptr(b_scale), _ptr(bias), _ptr(out),
                                           m, n, k, _stream()))
    return out


def mx_linear(x, b, b_scale, bias=None, fmt: int = MX_FMT_E2M1, scaling_mode="rceil", fuse: bool = True):
    """MXTensor's linear with a dynamic activation: to_mx(x, elem, 32, scaling_mode) then the MX GEMM.  x bf16 [M, K]; b / b_scale the
    weight as stored.  Shapes the streaming form takes run the cast inside the GEMM (ao_mx_dynamic_linear, bit-identical to the two
    launches); others cast first.  fuse=False: always the two launches."""
    dev = _require_gpu("mx_linear", x, b, b_scale, bias)
    if x.dtype != torch.bfloat16 or x.dim() != 2:
        raise RuntimeError(f"mx_linear: x must be a 2-D bfloat16 tensor, got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    m, kx = x.shape
    b, b_scale, bias, n, k = _mx_operands("mx_linear", fmt, b, b_scale, bias, kx)
    mode = _mx_mode(scaling_mode)
    if fuse and _lib.lib().ao_mx_dynamic_linear_fits(int(fmt), m, n, k):
        out = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
        if m > 0:
            with _on(dev):
                _lib.check(_lib.lib().ao_mx_dynamic_linear(int(fmt), _ptr(x), _ptr(b), _ptr(b_scale), _ptr(bias), _ptr(out), m, n, k, mode,
                                                           _stream()))
        return out
    if m == 0:
        return torch.empty((0, n), dtype=torch.bfloat16, device=dev)
    aq, a_s = mx_quantize(x, fmt, scaling_mode)
    return mx_mm(aq, a_s, b, b_scale, bias, fmt)


# ---- int8 / float8 weight-only linears (include/ao_mi355.h "WEIGHT-ONLY linears") ---------------------------------
WO8_FMT_INT8 = 0
WO8_FMT_E4M3 = 1
WO8_KERNELS = {0: "invalid", 1: "wo8_stream_kernel", 2: "wo8_tile_kernel"}


def wo8_route(fmt: int, m: int, n: int, k: int) -> dict:
    """The route int8_wo_linear / fp8_wo_linear launch for a shape (host logic only, ao_wo8_linear_route); kernel "invalid" for shapes
    nothing takes."""
    return _two_form_route("ao_wo8_linear_route", WO8_KERNELS, fmt, m, n, k)


def wo8_set_form(form: int) -> None:
    """Measurement only: 0 the product route, 1 the streaming form, 2 the tiled form (calling thread)."""
    _two_form_set_form("ao_wo8_linear_set_form", form)


def _wo_linear(name, fmt, x, wq, w_scale, bias, wdtype, out=None):
    dev = _require_gpu(name, x, wq, w_scale, bias)
    if x.dim() != 2 or x.dtype != torch.bfloat16:
        raise RuntimeError(f"{name}: x must be a 2-D bfloat16 tensor, got {tuple(x.shape)} {x.dtype}")
    if wq.dim() != 2 or wq.dtype != wdtype:
        raise RuntimeError(f"{name}: weight must be a 2-D {wdtype} tensor [N, K]")
    x = x.contiguous()
    wq = wq.contiguous()
    m, k = x.shape
    n, k2 = wq.shape
    if k != k2:
        raise RuntimeError(f"{name}: K mismatch {k} vs {k2}")
    w_scale = w_scale.reshape(-1).to(torch.float32).contiguous()
    if w_scale.numel() not in (n, 1):
        raise RuntimeError(f"{name}: weight scale must be per-row ([N]) or per-tensor (one element)")
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
        if bias.numel() != n:
            raise RuntimeError(f"{name}: bias must have N elements")
    if out is None:
        y = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    else:
        y = out
        if y.dtype != torch.bfloat16 or tuple(y.shape) != (m, n) or not y.is_contiguous() or y.device != dev:
            raise RuntimeError(f"{name}: out must be a contiguous bfloat16 [{m}, {n}] tensor on {dev}")
    with _on(dev):
        _lib.check(_lib.lib().ao_wo8_linear(fmt, _ptr(x), _ptr(wq.view(torch.uint8) if wdtype != torch.int8 else wq), _ptr(w_scale),
                                            w_scale.numel(), _ptr(bias), _ptr(y), m, n, k, _stream()))
    return y


def int8_wo_linear(x2, wq, w_scale, bias=None, out=None):
    """Int8Tensor WEIGHT-ONLY F.linear on a 2-D bf16 activation (int8_tensor.py:346-359): bf16(bf16(bf16(x . q^T) * bf16(s)) + bias),
    one launch, no activation cast.  w_scale: one per row or one element; out: an optional bf16 [M, N] tensor to write."""
    return _wo_linear("int8_wo_linear", WO8_FMT_INT8, x2, wq, w_scale, bias, torch.int8, out)


def fp8_wo_linear(x2, wq, w_scale, bias=None, out=None):
    """Float8Tensor WEIGHT-ONLY F.linear on a 2-D bf16 activation (float8_tensor.py:460-469): bf16(bf16(x . dequantize(w)^T) + bias)
    with the per-element bf16 rounding of dequantize (:255-275), one launch."""
    return _wo_linear("fp8_wo_linear", WO8_FMT_E4M3, x2, wq, w_scale, bias, torch.float8_e4m3fn, out)


__all__ += ["int8_wo_linear", "fp8_wo_linear", "wo8_route", "wo8_set_form"]


# ---- blockwise float8 linears: 1 x 128 activation blocks, 128 x 128 weight blocks (include/ao_mi355.h) ---------------
FP8_BLOCK_KERNELS = {0: "invalid", 1: "fp8_block_stream_kernel", 2: "fp8_block_tile_kernel"}
# The host rule for "the cast fused into the GEMM, or two launches": fused up to this many rows.  0: never by itself -- every one of
# the fused form's ceil(N / 16) workgroups casts the whole activation again, and at every M = 1 .. 15 on every one of the five Llama-3-8B
# shapes but o the one launch took longer than the two (tools/bench_fp8_block_linear.py --fused, profiles/fp8_block_linear.jsonl,
# DESIGN.md 4.12).  fuse=True still reaches it.
FP8_BLOCK_FUSED_MAX_ROWS = 0


def fp8_quantize_block_1x128(x: torch.Tensor):
    """Float8Tensor.from_hp(x, float8_e4m3fn, PerBlock([1, 128])) (float8_tensor.py:233-242, quant_primitives.py:2173-2212, :2271-2287).
    x bf16 [..., K], K % 128 == 0 -> (qdata float8_e4m3fn [..., K], scale fp32 [..., K/128]); no row-wide amax."""
    dev = _require_gpu("fp8_quantize_block_1x128", x)
    if x.dtype != torch.bfloat16 or x.dim() < 1 or x.shape[-1] % 128 != 0 or x.shape[-1] == 0:
        raise RuntimeError(f"fp8_quantize_block_1x128: x must be bfloat16 [..., K] with K a positive multiple of 128, got {x.dtype} {tuple(x.shape)}")
    k = x.shape[-1]
    rows = x.contiguous().reshape(-1, k)
    m = rows.shape[0]
    q = torch.empty((m, k), dtype=torch.uint8, device=dev)
    s = torch.empty((m, k // 128), dtype=torch.float32, device=dev)
    if m > 0:
        with _on(dev):
            _lib.check(_lib.lib().ao_fp8_quantize_block_1x128(_ptr(rows), _ptr(q), _ptr(s), m, k, _stream()))
    return q.view(torch.float8_e4m3fn).reshape(x.shape), s.reshape(*x.shape[:-1], k // 128)


def fp8_quantize_block_128x128(w: torch.Tensor):
    """Float8Tensor.from_hp(w, float8_e4m3fn, PerBlock([128, 128])) (same lines).  w bf16 [N, K], both multiples of 128 ->
    (qdata float8_e4m3fn [N, K], scale fp32 [N/128, K/128])."""
    dev = _require_gpu("fp8_quantize_block_128x128", w)
    if w.dtype != torch.bfloat16 or w.dim() != 2:
        raise RuntimeError(f"fp8_quantize_block_128x128: w must be a 2-D bfloat16 tensor, got {w.dtype} {tuple(w.shape)}")
    n, k = w.shape
    if n % 128 != 0 or k % 128 != 0 or k == 0:
        raise RuntimeError(f"fp8_quantize_block_128x128: shape {(n, k)} is not divisible by the block (128, 128)")
    w = w.contiguous()
    q = torch.empty((n, k), dtype=torch.uint8, device=dev)
    s = torch.empty((n // 128, k // 128), dtype=torch.float32, device=dev)
    if n > 0:
        with _on(dev):
            _lib.check(_lib.lib().ao_fp8_quantize_block_128x128(_ptr(w), _ptr(q), _ptr(s), n, k, _stream()))
    return q.view(torch.float8_e4m3fn), s


def fp8_block_linear_route(m: int, n: int, k: int) -> dict:
    """The route fp8_block_linear / fp8_block_mm launch for a shape (host logic only, ao_fp8_block_linear_route); kernel "invalid" for
    shapes nothing takes."""
    return _two_form_route("ao_fp8_block_linear_route", FP8_BLOCK_KERNELS, m, n, k)


def fp8_block_linear_kernel_name(m: int, n: int, k: int) -> str:
    return _two_form_kernel_name("ao_fp8_block_linear_kernel_name", m, n, k)


def fp8_block_linear_set_form(form: int) -> None:
    """Measurement only: 0 the product route, 1 the streaming form, 2 the tiled form (calling thread)."""
    _two_form_set_form("ao_fp8_block_linear_set_form", form)


def _fp8_block_weight(name, wq, w_scale, bias, k_from_a):
    wq = _fp8_bytes(name, wq)
    if wq.dim() != 2:
        raise RuntimeError(f"{name}: the weight codes must be 2-D [N, K], got {tuple(wq.shape)}")
    n, k = wq.shape
    if k != k_from_a:
        raise RuntimeError(f"{name}: K of the activation ({k_from_a}) and of the weight ({k}) differ")
    if k == 0 or k % 128 != 0:
        raise RuntimeError(f"{name}: K must be a positive multiple of 128, got {k}")
    if w_scale.dtype != torch.float32 or tuple(w_scale.shape) != ((n + 127) // 128, k // 128):
        raise RuntimeError(f"{name}: the weight scales must be float32 [ceil(N/128), K/128] = {((n + 127) // 128, k // 128)}, got "
                           f"{w_scale.dtype} {tuple(w_scale.shape)}")
    if bias is not None:
        if bias.numel() != n:
            raise RuntimeError(f"{name}: bias must have N elements")
        bias = bias.to(torch.bfloat16).contiguous()
    return wq.contiguous(), w_scale.contiguous(), bias, n, k


def _bf16_out(name, out, m, n, dev):
    if out is None:
        return torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    if out.dtype != torch.bfloat16 or tuple(out.shape) != (m, n) or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"{name}: out must be a contiguous bfloat16 [{m}, {n}] tensor on {dev}")
    return out


def fp8_block_mm(aq, a_scale, wq, w_scale, bias=None, out=None):
    """The blockwise GEMM on codes (kernels.py:56-128, float8_tensor.py:433-447): aq e4m3 [M, K], a_scale fp32 [M, K/128], wq e4m3 [N, K]
    (the weight as stored), w_scale fp32 [ceil(N/128), K/128], bias [N] -> bf16 [M, N] (ao_fp8_block_linear)."""
    dev = _require_gpu("fp8_block_mm", aq, a_scale, wq, w_scale, bias)
    aq = _fp8_bytes("fp8_block_mm", aq)
    if aq.dim() != 2:
        raise RuntimeError(f"fp8_block_mm: the activation codes must be 2-D [M, K], got {tuple(aq.shape)}")
    m = aq.shape[0]
    wq, w_scale, bias, n, k = _fp8_block_weight("fp8_block_mm", wq, w_scale, bias, aq.shape[1])
    if a_scale.dtype != torch.float32 or tuple(a_scale.shape) != (m, k // 128):
        raise RuntimeError(f"fp8_block_mm: the activation scales must be float32 [M, K/128] = {(m, k // 128)}, got {a_scale.dtype} {tuple(a_scale.shape)}")
    y = _bf16_out("fp8_block_mm", out, m, n, dev)
    if m > 0:
        with _on(dev):
            _lib.check(_lib.lib().ao_fp8_block_linear(_ptr(aq.contiguous()), _ptr(a_scale.contiguous()), _ptr(wq), _ptr(w_scale), _ptr(bias),
                                                      _ptr(y), m, n, k, _stream()))
    return y


def fp8_block_linear(x2, wq, w_scale, bias=None, fuse=None, out=None):
    """Float8Tensor's linear with 1 x 128 dynamic activation blocks on a 128 x 128 block-scaled weight (float8_tensor.py:433-447): the
    1 x 128 cast, then the blockwise GEMM.  x2 bf16 [M, K].  fuse None: the host rule (the cast inside the GEMM, one launch, up to
    FP8_BLOCK_FUSED_MAX_ROWS rows where the route is the streaming form; two launches otherwise); True: fused wherever the streaming
    form takes the shape; False: always two launches.  The same bits either way."""
    dev = _require_gpu("fp8_block_linear", x2, wq, w_scale, bias)
    if x2.dim() != 2 or x2.dtype != torch.bfloat16:
        raise RuntimeError(f"fp8_block_linear: x must be a 2-D bfloat16 tensor, got {tuple(x2.shape)} {x2.dtype}")
    x2 = x2.contiguous()
    m = x2.shape[0]
    wq, w_scale, bias, n, k = _fp8_block_weight("fp8_block_linear", wq, w_scale, bias, x2.shape[1])
    fused = (m <= FP8_BLOCK_FUSED_MAX_ROWS) if fuse is None else bool(fuse)
    if fused and m > 0 and _lib.lib().ao_fp8_block_dynamic_linear_fits(m, n, k):
        y = _bf16_out("fp8_block_linear", out, m, n, dev)
        with _on(dev):
            _lib.check(_lib.lib().ao_fp8_block_dynamic_linear(_ptr(x2), _ptr(wq), _ptr(w_scale), _ptr(bias), _ptr(y), m, n, k, _stream()))
        return y
    if m == 0:
        return _bf16_out("fp8_block_linear", out, m, n, dev)
    aq, a_s = fp8_quantize_block_1x128(x2)
    return fp8_block_mm(aq, a_s, wq, w_scale, bias, out)


__all__ += ["fp8_quantize_block_1x128", "fp8_quantize_block_128x128", "fp8_block_linear", "fp8_block_mm", "fp8_block_linear_kernel_name",
            "fp8_block_linear_route", "fp8_block_linear_set_form"]


# ---- blockwise float8 grouped GEMM for MoE experts (include/ao_mi355.h) ------------------------------------------------
FP8_BLOCK_GROUPED_KERNELS = {0: "invalid", 1: "fp8_block_grouped_stream_kernel", 2: "fp8_block_grouped_tile_kernel"}


def fp8_block_grouped_mm_route(m_total: int, n: int, k: int, e: int) -> dict:
    """The route fp8_block_grouped_mm launches for a shape (host logic only, ao_fp8_block_grouped_mm_route: it keys on the mean group
    size ceil(M_total / E)); kernel "invalid" for shapes nothing takes."""
    return _two_form_route("ao_fp8_block_grouped_mm_route", FP8_BLOCK_GROUPED_KERNELS, m_total, n, k, e)


def fp8_block_grouped_mm_kernel_name(m_total: int, n: int, k: int, e: int) -> str:
    return _two_form_kernel_name("ao_fp8_block_grouped_mm_kernel_name", m_total, n, k, e)


def fp8_block_grouped_mm_set_form(form: int) -> None:
    """Measurement only: 0 the product route, 1 the streaming form, 2 the tiled form (calling thread)."""
    _two_form_set_form("ao_fp8_block_grouped_mm_set_form", form)


def fp8_block_grouped_mm(aq, a_scale, wq, w_scale, offs, out=None):
    """The blockwise GEMM of fp8_block_mm per token group against that group's expert (ao_fp8_block_grouped_mm): aq e4m3 [M_total, K],
    a_scale fp32 [M_total, K/128], wq e4m3 [E, N, K] (the experts as stored), w_scale fp32 [E, ceil(N/128), K/128], offs int32 [E]
    cumulative group ends (read on the device) -> bf16 [M_total, N].  Rows past offs[-1] are not written: a fresh output is zero-filled,
    an `out=` tensor keeps what it held there."""
    name = "fp8_block_grouped_mm"
    dev = _require_gpu(name, aq, a_scale, wq, w_scale, offs, out)
    aq = _fp8_bytes(name, aq)
    wq = _fp8_bytes(name, wq)
    if aq.dim() != 2:
        raise RuntimeError(f"{name}: the activation codes must be 2-D [M_total, K], got {tuple(aq.shape)}")
    if wq.dim() != 3:
        raise RuntimeError(f"{name}: the weight codes must be 3-D [E, N, K], got {tuple(wq.shape)}")
    m, k = aq.shape
    e, n, kw = wq.shape
    if k != kw:
        raise RuntimeError(f"{name}: K of the activation ({k}) and of the weight ({kw}) differ")
    if k == 0 or k % 128 != 0:
        raise RuntimeError(f"{name}: K must be a positive multiple of 128, got {k}")
    if e < 1 or n < 1:
        raise RuntimeError(f"{name}: the weight codes must hold at least one expert and one row, got {tuple(wq.shape)}")
    if a_scale.dtype != torch.float32 or tuple(a_scale.shape) != (m, k // 128):
        raise RuntimeError(f"{name}: the activation scales must be float32 [M_total, K/128] = {(m, k // 128)}, got {a_scale.dtype} "
                           f"{tuple(a_scale.shape)}")
    if w_scale.dtype != torch.float32 or tuple(w_scale.shape) != (e, (n + 127) // 128, k // 128):
        raise RuntimeError(f"{name}: the weight scales must be float32 [E, ceil(N/128), K/128] = {(e, (n + 127) // 128, k // 128)}, got "
                           f"{w_scale.dtype} {tuple(w_scale.shape)}")
    if offs.dtype != torch.int32 or offs.dim() != 1 or offs.numel() != e:
        raise RuntimeError(f"{name}: offs must be int32 [E] = [{e}], got {offs.dtype} {tuple(offs.shape)}")
    if out is None:
        y = torch.zeros((m, n), dtype=torch.bfloat16, device=dev)
    else:
        y = _bf16_out(name, out, m, n, dev)
    if m > 0:
        with _on(dev):
            _lib.check(_lib.lib().ao_fp8_block_grouped_mm(_ptr(aq.contiguous()), _ptr(a_scale.contiguous()), _ptr(wq.contiguous()),
                                                          _ptr(w_scale.contiguous()), _ptr(offs.contiguous()), _ptr(y), m, n, k, e, _stream()))
    return y


__all__ += ["fp8_block_grouped_mm", "fp8_block_grouped_mm_route", "fp8_block_grouped_mm_kernel_name", "fp8_block_grouped_mm_set_form"]


# ---- blockwise float8 TRAINING: block-local casts and the weight-gradient GEMM (include/ao_mi355.h) --------------------
# The casts return e4m3fn codes and the fp32 RECIPROCAL scales fp8_block_mm / fp8_block_mm_wgrad multiply by.  Shapes and dtypes are
# checked first (ValueError naming the argument), then the device.
def _fp8_block_train_matrix(name, what, t, whole_rows):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16:
        raise ValueError(f"{name}: {what} must be a bfloat16 tensor, got {getattr(t, 'dtype', type(t))}")
    if t.dim() != 2:
        raise ValueError(f"{name}: {what} must be 2-D, got {t.dim()}-D {tuple(t.shape)}")
    r, c = t.shape
    if c % 128 != 0:
        raise ValueError(f"{name}: {what} has {c} columns, which must be a multiple of 128")
    if whole_rows and r % 128 != 0:
        raise ValueError(f"{name}: {what} has {r} rows, which must be a multiple of 128 for 128-row blocks")
    return r, c


def fp8_block_train_cast(x: torch.Tensor, rows: bool = True, cols: bool = False):
    """The blockwise training casts of an activation or a gradient (torchao/prototype/blockwise_fp8_training/kernels.py:1031-1118) in ONE
    read of x.  x bf16 [R, C], C % 128 == 0 -> (row, col):
      row = (q e4m3fn [R, C], inv fp32 [R, C/128]): 1 x 128 blocks (torch_blockwise_scale_act_quant_lhs), None without `rows`; any R;
      col = (q_t e4m3fn [C, R], inv fp32 [R/128, C]): 128 x 1 blocks stored transposed (torch_blockwise_scale_act_quant_rhs; the bytes of
            act_quant_transposed_lhs), None without `cols`; R % 128 == 0."""
    name = "fp8_block_train_cast"
    if not (rows or cols):
        raise ValueError(f"{name}: neither rows nor cols asked for")
    r, c = _fp8_block_train_matrix(name, "x", x, bool(cols))
    dev = _require_gpu(name, x)
    x = x.contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    q = inv = qt = invt = None
    if rows:
        q, inv = torch.empty((r, c), dtype=torch.uint8, device=dev), torch.empty((r, c // 128), **f32)
    if cols:
        qt, invt = torch.empty((c, r), dtype=torch.uint8, device=dev), torch.empty((r // 128, c), **f32)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_block_train_cast(_ptr(x), _ptr(q), _ptr(inv), _ptr(qt), _ptr(invt), r, c, _stream()))
    return ((q.view(torch.float8_e4m3fn), inv) if rows else None, (qt.view(torch.float8_e4m3fn), invt) if cols else None)


def fp8_block_train_cast_weight(w: torch.Tensor, transposed: Optional[bool] = False):
    """The 128 x 128 training cast of a weight (kernels.py:1121-1156, torch_blockwise_scale_weight_quant).  w bf16 [N, K], both multiples
    of 128 -> transposed False: (q e4m3fn [N, K], inv fp32 [N/128, K/128]); True: (q_t [K, N], inv_t [K/128, N/128]), the transposes (the
    operand of grad_input); None: both pairs from one read, (plain, transposed)."""
    name = "fp8_block_train_cast_weight"
    n, k = _fp8_block_train_matrix(name, "w", w, True)
    dev = _require_gpu(name, w)
    w = w.contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    q = inv = qt = invt = None
    if transposed is None or not transposed:
        q, inv = torch.empty((n, k), dtype=torch.uint8, device=dev), torch.empty((n // 128, k // 128), **f32)
    if transposed is None or transposed:
        qt, invt = torch.empty((k, n), dtype=torch.uint8, device=dev), torch.empty((k // 128, n // 128), **f32)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_block_train_cast_weight(_ptr(w), _ptr(q), _ptr(inv), _ptr(qt), _ptr(invt), n, k, _stream()))
    plain = (q.view(torch.float8_e4m3fn), inv) if q is not None else None
    trans = (qt.view(torch.float8_e4m3fn), invt) if qt is not None else None
    return (plain, trans) if transposed is None else (trans if transposed else plain)


def _fp8_block_wgrad_operands(name, g_t, g_inv, x_t, x_inv):
    """The shapes and dtypes of the column casts a blockwise weight gradient takes -> (M, N, K)."""
    for what, t in (("g_t", g_t), ("x_t", x_t)):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float8_e4m3fn, torch.uint8):
            raise ValueError(f"{name}: {what} must hold float8_e4m3fn codes (or their bytes as uint8), got {getattr(t, 'dtype', type(t))}")
        if t.dim() != 2:
            raise ValueError(f"{name}: {what} must be 2-D, got {t.dim()}-D {tuple(t.shape)}")
    n, m = g_t.shape
    k = x_t.shape[0]
    if x_t.shape[1] != m:
        raise ValueError(f"{name}: x_t must be [K, M={m}] like g_t [N, M], got {tuple(x_t.shape)}")
    for what, v in (("M (the columns of g_t)", m), ("N (the rows of g_t)", n), ("K (the rows of x_t)", k)):
        if v % 128 != 0:
            raise ValueError(f"{name}: {what} = {v} must be a multiple of 128")
    if n == 0 or k == 0:
        raise ValueError(f"{name}: g_t and x_t must have rows, got N={n} K={k}")
    for what, t, cols in (("g_inv", g_inv, n), ("x_inv", x_inv, k)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (m // 128, cols):
            raise ValueError(f"{name}: {what} must be float32 [M/128, {cols}] = {(m // 128, cols)}, got {getattr(t, 'dtype', type(t))} "
                             f"{tuple(getattr(t, 'shape', ()))}")
    return m, n, k


def fp8_block_mm_wgrad(g_t, g_inv, x_t, x_inv):
    """The blockwise weight gradient grad_output^T @ x (kernels.py:320-379) on the column casts of fp8_block_train_cast: g_t e4m3 [N, M],
    g_inv fp32 [M/128, N], x_t e4m3 [K, M], x_inv fp32 [M/128, K] -> bf16 [N, K];
    out[n][k] = bf16(sum over token blocks mb, ascending, of (p * g_inv[mb][n]) * x_inv[mb][k]), p the block's 128 products in fp32.
    M, N and K multiples of 128; M == 0 gives zeros."""
    name = "fp8_block_mm_wgrad"
    m, n, k = _fp8_block_wgrad_operands(name, g_t, g_inv, x_t, x_inv)
    dev = _require_gpu(name, g_t, g_inv, x_t, x_inv)
    g, x = _fp8_bytes(name, g_t).contiguous(), _fp8_bytes(name, x_t).contiguous()
    out = torch.empty((n, k), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_block_mm_wgrad(_ptr(g), _ptr(g_inv.contiguous()), _ptr(x), _ptr(x_inv.contiguous()), _ptr(out), m, n, k,
                                                    _stream()))
    return out


__all__ += ["fp8_block_train_cast", "fp8_block_train_cast_weight", "fp8_block_mm_wgrad"]


# ---- blockwise float8 TRAINING of the MoE grouped GEMM: the 3-D weight cast and the grouped weight gradient -----------
def fp8_block_train_cast_weight_3d(w: torch.Tensor, transposed: Optional[bool] = False):
    """fp8_block_train_cast_weight over a stack of experts in one launch (ao_fp8_block_train_cast_weight_3d).  w bf16 [E, N, K], N and K
    multiples of 128 -> transposed False: (q e4m3fn [E, N, K], inv fp32 [E, N/128, K/128]); True: (q_t [E, K, N], inv_t [E, K/128, N/128]);
    None: both pairs from one read, (plain, transposed).  Expert e's outputs are the bytes of the 2-D op on w[e]."""
    name = "fp8_block_train_cast_weight_3d"
    if not isinstance(w, torch.Tensor) or w.dtype != torch.bfloat16:
        raise ValueError(f"{name}: w must be a bfloat16 tensor, got {getattr(w, 'dtype', type(w))}")
    if w.dim() != 3:
        raise ValueError(f"{name}: w must be 3-D [E, N, K], got {w.dim()}-D {tuple(w.shape)}")
    e, n, k = w.shape
    if n % 128 != 0:
        raise ValueError(f"{name}: w has {n} rows an expert, which must be a multiple of 128")
    if k % 128 != 0:
        raise ValueError(f"{name}: w has {k} columns, which must be a multiple of 128")
    if e > 65535 or e * (n // 128) > 65535:
        raise ValueError(f"{name}: w holds E={e} experts of {n // 128} row tiles; at most 65535 experts and 65535 row tiles fit one launch")
    dev = _require_gpu(name, w)
    w = w.contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    q = inv = qt = invt = None
    if transposed is None or not transposed:
        q, inv = torch.empty((e, n, k), dtype=torch.uint8, device=dev), torch.empty((e, n // 128, k // 128), **f32)
    if transposed is None or transposed:
        qt, invt = torch.empty((e, k, n), dtype=torch.uint8, device=dev), torch.empty((e, k // 128, n // 128), **f32)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_block_train_cast_weight_3d(_ptr(w), _ptr(q), _ptr(inv), _ptr(qt), _ptr(invt), e, n, k, _stream()))
    plain = (q.view(torch.float8_e4m3fn), inv) if q is not None else None
    trans = (qt.view(torch.float8_e4m3fn), invt) if qt is not None else None
    return (plain, trans) if transposed is None else (trans if transposed else plain)


def fp8_block_grouped_mm_wgrad(g_t, g_inv, x_t, x_inv, offs):
    """The blockwise weight gradient per token group (ao_fp8_block_grouped_mm_wgrad) on the column casts of fp8_block_train_cast over ALL
    tokens: g_t e4m3 [N, M], g_inv fp32 [M/128, N], x_t e4m3 [K, M], x_inv fp32 [M/128, K], offs int32 [E] cumulative group ends (read on
    the device; None: one group of every token) -> bf16 [E, N, K];
    out[e][n][k] = bf16(sum over the token blocks mb that meet group e, ascending, of (p * g_inv[mb][n]) * x_inv[mb][k]), p the products of
    the block's tokens inside the group.  M, N and K multiples of 128; group ends need no alignment; an empty group gives zeros."""
    name = "fp8_block_grouped_mm_wgrad"
    m, n, k = _fp8_block_wgrad_operands(name, g_t, g_inv, x_t, x_inv)
    if offs is not None and (not isinstance(offs, torch.Tensor) or offs.dtype != torch.int32 or offs.dim() != 1 or offs.numel() == 0):
        raise ValueError(f"{name}: offs must be a non-empty int32 [E] tensor or None, got {getattr(offs, 'dtype', type(offs))} "
                         f"{tuple(getattr(offs, 'shape', ()))}")
    e = 1 if offs is None else offs.numel()
    if e > 65535:
        raise ValueError(f"{name}: offs holds {e} groups; at most 65535 fit one launch")
    if n * m >= 2 ** 31 or k * m >= 2 ** 31:
        raise ValueError(f"{name}: g_t and x_t must each be below 2^31 bytes, got N M = {n * m} and K M = {k * m}")
    dev = _require_gpu(name, g_t, g_inv, x_t, x_inv, offs)
    g, x = _fp8_bytes(name, g_t).contiguous(), _fp8_bytes(name, x_t).contiguous()
    out = torch.empty((e, n, k), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_fp8_block_grouped_mm_wgrad(_ptr(g), _ptr(g_inv.contiguous()), _ptr(x), _ptr(x_inv.contiguous()),
                                                            _ptr(None if offs is None else offs.contiguous()), _ptr(out), m, n, k, e, _stream()))
    return out


__all__ += ["fp8_block_train_cast_weight_3d", "fp8_block_grouped_mm_wgrad"]


# ---- NVFP4 linears: e2m1 codes, 1 x 16 e4m3 block scales, fp32 per-tensor scales (include/ao_mi355.h "NVFP4 linears") ----
NVFP4_KIND_WEIGHT_ONLY = 0
NVFP4_KIND_DYNAMIC = 1
NVFP4_KERNELS = {0: "invalid", 1: "nvfp4_stream_kernel", 2: "nvfp4_tile_kernel"}


def nvfp4_linear_route(kind: int, m: int, n: int, k: int) -> dict:
    """The route nvfp4_wo_linear (kind 0) / nvfp4_mm (kind 1) launch for a shape (host logic only, ao_nvfp4_linear_route); kernel
    "invalid" for shapes nothing takes."""
    return _two_form_route("ao_nvfp4_linear_route", NVFP4_KERNELS, kind, m, n, k)


def nvfp4_linear_kernel_name(kind: int, m: int, n: int, k: int) -> str:
    return _two_form_kernel_name("ao_nvfp4_linear_kernel_name", kind, m, n, k)


def nvfp4_set_form(form: int) -> None:
    """Measurement only: 0 the product route, 1 the streaming form, 2 the tiled form (calling thread)."""
    _two_form_set_form("ao_nvfp4_linear_set_form", form)


def _nvfp4_rows(name, x):
    if x.dtype != torch.bfloat16:
        raise RuntimeError(f"{name}: expected bfloat16, got {x.dtype}")
    if x.dim() < 1 or not x.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    c = x.shape[-1]
    if c % 16 != 0 or c == 0:
        raise RuntimeError(f"{name}: the last dimension of shape {tuple(x.shape)} must be divisible by 16")
    return x.numel() // c, c


def _nvfp4_scalar(name, what, p, dev):
    """A per-tensor scale as one fp32 on the device (None stays None): read by the kernels through its pointer, never on the host."""
    if p is None:
        return None
    if not isinstance(p, torch.Tensor) or p.numel() != 1:
        raise RuntimeError(f"{name}: {what} must be a tensor of one element")
    if p.device != dev:
        raise RuntimeError(f"{name}: {what} is on {p.device}, the operands on {dev}")
    return p.reshape(()).to(torch.float32).contiguous()


def nvfp4_amax_scale(x: torch.Tensor) -> torch.Tensor:
    """per_tensor_amax_to_scale(torch.max(torch.abs(x))) (nvfp4_tensor.py:605-607, :756-769) on the device: bf16 [..., C] -> fp32
    0-dim max|x| / 2688, NaN if x holds one.  No host read (capturable)."""
    dev = _require_gpu("nvfp4_amax_scale", x)
    r, c = _nvfp4_rows("nvfp4_amax_scale", x)
    out = torch.empty((), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nvfp4_amax_scale(_ptr(x), _ptr(out), r, c, _stream()))
    return out


def nvfp4_quantize(x: torch.Tensor, per_tensor_scale: Optional[torch.Tensor] = None):
    """nvfp4_quantize (nvfp4_tensor.py:772-854), the reference's bytes.  x bf16 [..., C] -> (codes uint8 [..., C/2], element 2i in the low
    nibble; block scales float8_e4m3fn [..., C/16], row-major).  per_tensor_scale: a one-element tensor on the device, or None."""
    dev = _require_gpu("nvfp4_quantize", x, per_tensor_scale)
    r, c = _nvfp4_rows("nvfp4_quantize", x)
    p = _nvfp4_scalar("nvfp4_quantize", "per_tensor_scale", per_tensor_scale, dev)
    q = torch.empty((*x.shape[:-1], c // 2), dtype=torch.uint8, device=dev)
    s = torch.empty((*x.shape[:-1], c // 16), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nvfp4_quantize(_ptr(x), _ptr(p), _ptr(q), _ptr(s), r, c, _stream()))
    return q, s.view(torch.float8_e4m3fn)


def _nvfp4_codes(name, what, q, s):
    q = q.view(torch.uint8) if q.dtype == torch.float4_e2m1fn_x2 else q
    if q.dtype != torch.uint8 or q.dim() != 2:
        raise RuntimeError(f"{name}: the {what} codes must be a 2-D uint8 tensor [rows, K/2], got {q.dtype} {tuple(q.shape)}")
    rows, k = q.shape[0], q.shape[1] * 2
    if s.dtype not in (torch.float8_e4m3fn, torch.uint8):
        raise RuntimeError(f"{name}: the {what} block scales must be float8_e4m3fn, got {s.dtype}")
    s = s.view(torch.uint8)
    if k % 16 != 0 or tuple(s.shape) != (rows, k // 16):
        raise RuntimeError(f"{name}: the {what} block scales must be row-major [rows, K/16] = {(rows, k // 16)}, got {tuple(s.shape)}")
    return q.contiguous(), s.contiguous(), rows, k


def _nvfp4_bias(name, bias, n):
    if bias is None:
        return None
    if bias.dtype != torch.bfloat16 or bias.numel() != n:
        raise RuntimeError(f"{name}: bias must be bfloat16 [N], got {bias.dtype} {tuple(bias.shape)}")
    return bias.contiguous()


def nvfp4_wo_linear(x2, wq, w_scale, per_tensor_scale=None, bias=None, out=None):
    """NVFP4Tensor's WEIGHT-ONLY F.linear on a 2-D bf16 activation (nvfp4_tensor.py:593-596): bf16(x . bf16(dequantize(w))^T + bias), fp32
    accumulation, one rounding; one launch that reads 0.5625 bytes a weight.  wq [N, K/2], w_scale e4m3 [N, K/16], per_tensor_scale one
    fp32 on the device or None; out: an optional bf16 [M, N] tensor to write."""
    dev = _require_gpu("nvfp4_wo_linear", x2, wq, w_scale, per_tensor_scale, bias)
    if x2.dim() != 2 or x2.dtype != torch.bfloat16:
        raise RuntimeError(f"nvfp4_wo_linear: x must be a 2-D bfloat16 tensor, got {tuple(x2.shape)} {x2.dtype}")
    x2 = x2.contiguous()
    wq, w_scale, n, k = _nvfp4_codes("nvfp4_wo_linear", "weight", wq, w_scale)
    m, kx = x2.shape
    if kx != k:
        raise RuntimeError(f"nvfp4_wo_linear: K mismatch {kx} vs {k}")
    p = _nvfp4_scalar("nvfp4_wo_linear", "per_tensor_scale", per_tensor_scale, dev)
    bias = _nvfp4_bias("nvfp4_wo_linear", bias, n)
    y = _bf16_out("nvfp4_wo_linear", out, m, n, dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nvfp4_wo_linear(_ptr(x2), _ptr(wq), _ptr(w_scale), _ptr(p), _ptr(bias), _ptr(y), m, n, k, _stream()))
    return y


def nvfp4_mm(a, a_scale, b, b_scale, a_per_tensor_scale=None, b_per_tensor_scale=None, bias=None, out=None):
    """The NVFP4 x NVFP4 GEMM on codes (_addmm_nvfp4_dispatch, nvfp4_tensor.py:487-578): a [M, K/2], a_scale [M, K/16], b [N, K/2] (the
    weight as stored), b_scale [N, K/16] -> bf16 [M, N].  acc = sum_k dq(a) dq(b) in fp32; without per-tensor scales bf16(acc + bias),
    otherwise bf16(bf16(bf16(acc) bf16(P)) + bias) with P = pa pb."""
    dev = _require_gpu("nvfp4_mm", a, a_scale, b, b_scale, a_per_tensor_scale, b_per_tensor_scale, bias)
    a, a_scale, m, ka = _nvfp4_codes("nvfp4_mm", "activation", a, a_scale)
    b, b_scale, n, k = _nvfp4_codes("nvfp4_mm", "weight", b, b_scale)
    if ka != k:
        raise RuntimeError(f"nvfp4_mm: K of the activation ({ka}) and of the weight ({k}) differ")
    pa = _nvfp4_scalar("nvfp4_mm", "a_per_tensor_scale", a_per_tensor_scale, dev)
    pb = _nvfp4_scalar("nvfp4_mm", "b_per_tensor_scale", b_per_tensor_scale, dev)
    bias = _nvfp4_bias("nvfp4_mm", bias, n)
    y = _bf16_out("nvfp4_mm", out, m, n, dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nvfp4_linear(_ptr(a), _ptr(a_scale), _ptr(pa), _ptr(b), _ptr(b_scale), _ptr(pb), _ptr(bias), _ptr(y), m, n, k,
                                              _stream()))
    return y


def nvfp4_linear(x2, wq, w_scale, w_per_tensor_scale=None, act_per_tensor_scale=None, dynamic_per_tensor_scale=False, bias=None):
    """NVFP4Tensor's F.linear with a dynamic activation (nvfp4_tensor.py:598-619): the activation's per-tensor scale (the device amax when
    dynamic_per_tensor_scale, else act_per_tensor_scale, else none), its 1 x 16 cast, then the codes x codes GEMM."""
    pa = nvfp4_amax_scale(x2) if dynamic_per_tensor_scale else act_per_tensor_scale
    aq, a_s = nvfp4_quantize(x2.contiguous(), pa)
    return nvfp4_mm(aq, a_s, wq, w_scale, pa, w_per_tensor_scale, bias)


__all__ += ["nvfp4_amax_scale", "nvfp4_quantize", "nvfp4_wo_linear", "nvfp4_mm", "nvfp4_linear", "nvfp4_linear_route",
            "nvfp4_linear_kernel_name", "nvfp4_set_form"]


# ---- NVFP4 grouped GEMM for MoE experts (include/ao_mi355.h "NVFP4 grouped GEMM") -----------------------------------------
NVFP4_GROUPED_KERNELS = {0: "invalid", 1: "nvfp4_grouped_stream_kernel", 2: "nvfp4_grouped_tile_kernel"}


def nvfp4_grouped_mm_route(kind: int, m_total: int, n: int, k: int, e: int) -> dict:
    """The route nvfp4_grouped_mm launches for a kind and shape (host logic only, ao_nvfp4_grouped_mm_route: it keys on the mean group
    size ceil(M_total / E)); kernel "invalid" for shapes nothing takes."""
    return _two_form_route("ao_nvfp4_grouped_mm_route", NVFP4_GROUPED_KERNELS, kind, m_total, n, k, e)


def nvfp4_grouped_mm_kernel_name(kind: int, m_total: int, n: int, k: int, e: int) -> str:
    return _two_form_kernel_name("ao_nvfp4_grouped_mm_kernel_name", kind, m_total, n, k, e)


def nvfp4_grouped_mm_set_form(form: int) -> None:
    """Measurement only: 0 the product route, 1 the streaming form, 2 the tiled form (calling thread)."""
    _two_form_set_form("ao_nvfp4_grouped_mm_set_form", form)


def _nvfp4_offs(name, offs, e):
    if offs.dtype != torch.int32 or offs.dim() != 1 or offs.numel() != e:
        raise RuntimeError(f"{name}: offs must be int32 [E] = [{e}], got {offs.dtype} {tuple(offs.shape)}")
    return offs.contiguous()


def _nvfp4_expert_scales(name, what, p, e, dev):
    """Per-expert (per-group) scales as fp32 [E] on the device (None stays None): read by the kernels, never on the host."""
    if p is None:
        return None
    if not isinstance(p, torch.Tensor) or p.numel() != e:
        raise RuntimeError(f"{name}: {what} must be a tensor of E = {e} elements, one an expert, got "
                           f"{tuple(p.shape) if isinstance(p, torch.Tensor) else type(p).__name__}")
    if p.device != dev:
        raise RuntimeError(f"{name}: {what} is on {p.device}, the operands on {dev}")
    return p.reshape(e).to(torch.float32).contiguous()


def _nvfp4_expert_codes(name, q, s):
    q = q.view(torch.uint8) if q.dtype == torch.float4_e2m1fn_x2 else q
    if q.dtype != torch.uint8 or q.dim() != 3:
        raise RuntimeError(f"{name}: the weight codes must be a 3-D uint8 tensor [E, N, K/2], got {q.dtype} {tuple(q.shape)}")
    e, n, k = q.shape[0], q.shape[1], q.shape[2] * 2
    if e < 1 or n < 1:
        raise RuntimeError(f"{name}: the weight codes must hold at least one expert and one row, got {tuple(q.shape)}")
    if s.dtype not in (torch.float8_e4m3fn, torch.uint8):
        raise RuntimeError(f"{name}: the weight block scales must be float8_e4m3fn, got {s.dtype}")
    s = s.view(torch.uint8)
    if k == 0 or k % 16 != 0 or tuple(s.shape) != (e, n, k // 16):
        raise RuntimeError(f"{name}: the weight block scales must be row-major [E, N, K/16] = {(e, n, k // 16)}, got {tuple(s.shape)}")
    return q.contiguous(), s.contiguous(), e, n, k


def nvfp4_group_amax_scale(x: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """nvfp4_amax_scale per token group (ao_nvfp4_group_amax_scale): x bf16 [M_total, K], offs int32 [E] cumulative group ends -> fp32 [E],
    max|x[group e]| / 2688 (NaN if the group holds one, 0 for an empty group).  No host read (capturable)."""
    name = "nvfp4_group_amax_scale"
    dev = _require_gpu(name, x, offs)
    if x.dim() != 2:
        raise RuntimeError(f"{name}: x must be 2-D [M_total, K], got {tuple(x.shape)}")
    r, c = _nvfp4_rows(name, x)
    offs = _nvfp4_offs(name, offs, offs.numel() if offs.dim() == 1 else -1)
    e = offs.numel()
    out = torch.empty((e,), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nvfp4_group_amax_scale(_ptr(x), _ptr(offs), _ptr(out), r, c, e, _stream()))
    return out


def nvfp4_quantize_grouped(x: torch.Tensor, per_group_scale: Optional[torch.Tensor], offs: torch.Tensor):
    """nvfp4_quantize with row r cast under per_group_scale[e] of the group that holds it (ao_nvfp4_quantize_grouped): x bf16 [M_total, K],
    per_group_scale fp32 [E] on the device or None, offs int32 [E] -> (codes uint8 [M_total, K/2], block scales float8_e4m3fn
    [M_total, K/16]).  Rows past offs[-1] are not cast: they are zero in the fresh outputs."""
    name = "nvfp4_quantize_grouped"
    dev = _require_gpu(name, x, per_group_scale, offs)
    if x.dim() != 2:
        raise RuntimeError(f"{name}: x must be 2-D [M_total, K], got {tuple(x.shape)}")
    r, c = _nvfp4_rows(name, x)
    offs = _nvfp4_offs(name, offs, offs.numel() if offs.dim() == 1 else -1)
    e = offs.numel()
    p = _nvfp4_expert_scales(name, "per_group_scale", per_group_scale, e, dev)
    q = torch.zeros((r, c // 2), dtype=torch.uint8, device=dev)
    s = torch.zeros((r, c // 16), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nvfp4_quantize_grouped(_ptr(x), _ptr(p), _ptr(offs), _ptr(q), _ptr(s), r, c, e, _stream()))
    return q, s.view(torch.float8_e4m3fn)


def nvfp4_grouped_mm(kind, a, a_scale, wq, w_scale, offs, a_per_group_scale=None, w_per_expert_scale=None, out=None):
    """The NVFP4 chains per token group against that group's expert (ao_nvfp4_grouped_mm), no bias.
    kind NVFP4_KIND_WEIGHT_ONLY: a bf16 [M_total, K], a_scale None; nvfp4_wo_linear per group.
    kind NVFP4_KIND_DYNAMIC: a codes [M_total, K/2], a_scale e4m3 [M_total, K/16]; nvfp4_mm per group.
    wq codes [E, N, K/2] (the experts as stored), w_scale e4m3 [E, N, K/16], offs int32 [E] cumulative group ends (read on the device),
    a_per_group_scale / w_per_expert_scale fp32 [E] on the device or None -> bf16 [M_total, N].  Rows past offs[-1] are not written: a fresh
    output is zero-filled, an `out=` tensor keeps what it held there."""
    name = "nvfp4_grouped_mm"
    dev = _require_gpu(name, a, a_scale, wq, w_scale, offs, a_per_group_scale, w_per_expert_scale, out)
    wq, w_scale, e, n, k = _nvfp4_expert_codes(name, wq, w_scale)
    if kind == NVFP4_KIND_WEIGHT_ONLY:
        if a.dim() != 2 or a.dtype != torch.bfloat16:
            raise RuntimeError(f"{name}: the weight-only activation must be a 2-D bfloat16 tensor, got {tuple(a.shape)} {a.dtype}")
        if a_scale is not None or a_per_group_scale is not None:
            raise RuntimeError(f"{name}: the weight-only kind takes no activation scales")
        x, aq, a_s = a.contiguous(), None, None
        m, ka = x.shape
    elif kind == NVFP4_KIND_DYNAMIC:
        if a_scale is None:
            raise RuntimeError(f"{name}: the codes x codes kind needs the activation block scales")
        aq, a_s, m, ka = _nvfp4_codes(name, "activation", a, a_scale)
        x = None
    else:
        raise RuntimeError(f"{name}: kind must be NVFP4_KIND_WEIGHT_ONLY (0) or NVFP4_KIND_DYNAMIC (1), got {kind}")
    if ka != k:
        raise RuntimeError(f"{name}: K of the activation ({ka}) and of the weight ({k}) differ")
    offs = _nvfp4_offs(name, offs, e)
    pa = _nvfp4_expert_scales(name, "a_per_group_scale", a_per_group_scale, e, dev)
    pb = _nvfp4_expert_scales(name, "w_per_expert_scale", w_per_expert_scale, e, dev)
    if out is None:
        y = torch.zeros((m, n), dtype=torch.bfloat16, device=dev)
    else:
        y = _bf16_out(name, out, m, n, dev)
    if m > 0:
        with _on(dev):
            _lib.check(_lib.lib().ao_nvfp4_grouped_mm(int(kind), _ptr(x), _ptr(aq), _ptr(a_s), _ptr(wq), _ptr(w_scale), _ptr(pa), _ptr(pb),
                                                      _ptr(offs), _ptr(y), m, n, k, e, _stream()))
    return y


__all__ += ["nvfp4_grouped_mm", "nvfp4_group_amax_scale", "nvfp4_quantize_grouped", "nvfp4_grouped_mm_route",
            "nvfp4_grouped_mm_kernel_name", "nvfp4_grouped_mm_set_form"]


# ---- NVFP4 training: casts and the scaled_mm epilogue (include/ao_mi355.h "NVFP4 training") -------------------------------
def nvfp4_sign_mask(sign_vector) -> int:
    """The 16-point Hadamard sign vector as the C ABI's 16-bit mask: bit i set means s_i = -1.  Takes 16 values of +-1 (a sequence or a
    tensor) or a mask already."""
    if isinstance(sign_vector, int):
        if not 0 <= sign_vector < 1 << 16:
            raise ValueError(f"sign mask must be a 16-bit mask, got {sign_vector:#x}")
        return sign_vector
    vals = [int(v) for v in (sign_vector.detach().cpu().tolist() if isinstance(sign_vector, torch.Tensor) else sign_vector)]
    if len(vals) != 16 or any(v not in (1, -1) for v in vals):
        raise ValueError(f"the RHT sign vector must be 16 values of +1 or -1, got {vals}")
    return sum(1 << i for i, v in enumerate(vals) if v < 0)


def _nvfp4_train_matrix(name, x):
    if x.dtype != torch.bfloat16 or x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous 2-D bfloat16 tensor, got {x.dtype} {tuple(x.shape)}")
    m, n = x.shape
    if m % 16 != 0 or n % 16 != 0 or n == 0:
        raise RuntimeError(f"{name}: both dimensions of shape {tuple(x.shape)} must be divisible by 16")
    return m, n


def _nvfp4_train_out(name, what, out, rows, cols, dev):
    """(codes uint8 [rows, cols/2], scale bytes uint8 [rows, cols/16]): fresh, or the caller's pair checked"""
    if out is None:
        return (torch.empty((rows, cols // 2), dtype=torch.uint8, device=dev), torch.empty((rows, cols // 16), dtype=torch.uint8, device=dev))
    q, s = out
    for t, shape in ((q, (rows, cols // 2)), (s, (rows, cols // 16))):
        if t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f"{name}: the {what} output must be contiguous uint8 {shape} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return q, s


def _nvfp4_i64(name, what, t, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.numel() != 1 or t.device != dev:
        raise RuntimeError(f"{name}: {what} must be an int64 tensor of one element on {dev}")
    return t.contiguous()


def nvfp4_train_amax(x: torch.Tensor, sign_vector, want_rht: bool = True) -> torch.Tensor:
    """triton_rht_amax (nvfp4_training/hadamard_amax_triton.py): x bf16 [M, N] -> fp32 [2] on the device, [0] = max|bf16(RHT(x^T))| (0 when
    not want_rht), [1] = max|x|.  No host read (capturable)."""
    name = "nvfp4_train_amax"
    dev = _require_gpu(name, x)
    m, n = _nvfp4_train_matrix(name, x)
    mask = nvfp4_sign_mask(sign_vector)
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nvfp4_train_amax(_ptr(x), _ptr(out), m, n, mask, int(bool(want_rht)), _stream()))
    return out


def nvfp4_train_quantize_row_col(x: torch.Tensor, amax2: torch.Tensor, sign_vector, sr_seed: Optional[torch.Tensor] = None,
                                 col_offset: Optional[torch.Tensor] = None, row_offset: Optional[torch.Tensor] = None, *, want_col: bool = True,
                                 want_row: bool = True, col_out=None, row_out=None):
    """triton_rht_quantize_row_col (nvfp4_training/hadamard_quantize_row_col_triton.py) in one read of x bf16 [M, N]: returns
    (col_q [N, M/2], col_s e4m3 [N, M/16], row_q [M, N/2], row_s e4m3 [M, N/16]) -- the 1 x 16 cast of bf16(RHT(x^T)) under amax2[0] and of x
    under amax2[1], the scales row-major; a direction not wanted is (None, None).  sr_seed None: round to nearest even; otherwise stochastic
    rounding of both outputs from the int64 device tensors sr_seed, col_offset, row_offset (quant_math.h "NVFP4 training")."""
    name = "nvfp4_train_quantize_row_col"
    dev = _require_gpu(name, x, amax2, sr_seed, col_offset, row_offset)
    m, n = _nvfp4_train_matrix(name, x)
    mask = nvfp4_sign_mask(sign_vector)
    if not (want_col or want_row):
        raise RuntimeError(f"{name}: neither output is wanted")
    if not isinstance(amax2, torch.Tensor) or amax2.dtype != torch.float32 or amax2.numel() != 2 or not amax2.is_contiguous():
        raise RuntimeError(f"{name}: amax2 must be a contiguous float32 tensor of two elements (column amax, row amax)")
    if sr_seed is not None:
        sr_seed = _nvfp4_i64(name, "sr_seed", sr_seed, dev)
        col_offset = _nvfp4_i64(name, "col_offset", col_offset, dev) if want_col else None
        row_offset = _nvfp4_i64(name, "row_offset", row_offset, dev) if want_row else None
    else:
        col_offset = row_offset = None
    cq, cs = _nvfp4_train_out(name, "column", col_out, n, m, dev) if want_col else (None, None)
    rq, rs = _nvfp4_train_out(name, "row", row_out, m, n, dev) if want_row else (None, None)
    with _on(dev):
        _lib.check(_lib.lib().ao_nvfp4_train_quantize_row_col(_ptr(x), _ptr(amax2), mask, _ptr(sr_seed), _ptr(col_offset), _ptr(row_offset),
                                                              _ptr(cq), _ptr(cs), _ptr(rq), _ptr(rs), m, n, _stream()))
    f8 = torch.float8_e4m3fn
    return cq, (None if cs is None else cs.view(f8)), rq, (None if rs is None else rs.view(f8))


def nvfp4_train_quantize_weight_2d(w: torch.Tensor, amax: torch.Tensor, *, out=None, out_t=None):
    """triton_weight_quantize_2d (nvfp4_training/quantize_2d_triton.py): w bf16 [N, K] under 16 x 16 block scales, round to nearest even,
    amax = max|w| as one fp32 on the device -> (q [N, K/2], s e4m3 [N, K/16], qt [K, N/2], st e4m3 [K, N/16]): the cast of w and, from the
    same read and the same block scales, of w^T."""
    name = "nvfp4_train_quantize_weight_2d"
    dev = _require_gpu(name, w, amax)
    n, k = _nvfp4_train_matrix(name, w)
    a = _nvfp4_scalar(name, "amax", amax, dev)
    q, s = _nvfp4_train_out(name, "weight", out, n, k, dev)
    qt, st = _nvfp4_train_out(name, "transposed weight", out_t, k, n, dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nvfp4_train_quantize_weight_2d(_ptr(w), _ptr(a), _ptr(q), _ptr(s), _ptr(qt), _ptr(st), n, k, _stream()))
    return q, s.view(torch.float8_e4m3fn), qt, st.view(torch.float8_e4m3fn)


def nvfp4_scaled_mm(a, a_scale, b, b_scale, a_per_tensor_scale, b_per_tensor_scale, out=None):
    """torch.nn.functional.scaled_mm on e2m1 codes with BlockWise1x16 + TensorWise scales (nvfp4_training/nvfp4_linear.py:213-223): a
    [M, K/2], a_scale [M, K/16], b [N, K/2], b_scale [N, K/16], both per-tensor scales one fp32 on the device -> bf16 [M, N] =
    bf16(acc (pa pb)): fp32 accumulation, the scales' product in fp32, ONE rounding, no bias (nvfp4_mm rounds acc and P to bf16 first)."""
    name = "nvfp4_scaled_mm"
    dev = _require_gpu(name, a, a_scale, b, b_scale, a_per_tensor_scale, b_per_tensor_scale, out)
    a, a_scale, m, ka = _nvfp4_codes(name, "activation", a, a_scale)
    b, b_scale, n, k = _nvfp4_codes(name, "weight", b, b_scale)
    if ka != k:
        raise RuntimeError(f"{name}: K of the activation ({ka}) and of the weight ({k}) differ")
    pa = _nvfp4_scalar(name, "a_per_tensor_scale", a_per_tensor_scale, dev)
    pb = _nvfp4_scalar(name, "b_per_tensor_scale", b_per_tensor_scale, dev)
    if pa is None or pb is None:
        raise RuntimeError(f"{name}: both per-tensor scales are required")
    y = _bf16_out(name, out, m, n, dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nvfp4_scaled_mm(_ptr(a), _ptr(a_scale), _ptr(pa), _ptr(b), _ptr(b_scale), _ptr(pb), _ptr(y), m, n, k, _stream()))
    return y


__all__ += ["nvfp4_sign_mask", "nvfp4_train_amax", "nvfp4_train_quantize_row_col", "nvfp4_train_quantize_weight_2d", "nvfp4_scaled_mm"]


# ---------------------------------------------------------------------------
# Quantization-aware training (torchao.quantization.qat): each fake quantizer and its gradient as one launch, bf16 -> bf16.  The backward
# ops take the forward's INPUT and the incoming gradient; nothing else is saved.
# ---------------------------------------------------------------------------
def _qat_bf16(name, what, t):
    if t.dtype != torch.bfloat16:
        raise RuntimeError(f"{name}: {what} must be bfloat16, got {t.dtype}")


def _qat_int4_args(name, w, group_size, grad_out=None):
    _qat_bf16(name, "w", w)
    if w.dim() != 2:
        raise RuntimeError(f"{name}: w must be 2-D [N, K], got {w.dim()}-D")
    if group_size not in (32, 64, 128, 256):
        raise ValueError(f"{name}: group_size must be one of 32, 64, 128, 256, got {group_size}")
    n, k = w.shape
    if k == 0 or k % group_size != 0:
        raise ValueError(f"{name}: K={k} must be a multiple of group_size={group_size}")
    if grad_out is not None:
        _qat_bf16(name, "grad_out", grad_out)
        if grad_out.shape != w.shape:
            raise RuntimeError(f"{name}: grad_out has shape {tuple(grad_out.shape)} but w has {tuple(w.shape)}")
        grad_out = grad_out.contiguous()
    dev = _require_gpu(name, w, grad_out)
    return dev, w.contiguous(), grad_out, n, k


def qat_int4_fake_quantize(w: torch.Tensor, group_size: int = 128) -> torch.Tensor:
    """Int4WeightFakeQuantizer._bf16_activations_forward (torchao/quantization/qat/fake_quantizer.py:167-187): w bf16 [N, K] -> bf16 [N, K],
    every group of `group_size` along K replaced by the values its asymmetric int4 codes stand for: s = max(max - min, 1e-6) / 15,
    q = clamp(rint((w - min) / s), 0, 15), out = (q - 8) s + (min + 8 s), in fp32.  The codes are int4_plain_quantize's."""
    name = "qat_int4_fake_quantize"
    dev, w, _, n, k = _qat_int4_args(name, w, group_size)
    out = torch.empty_like(w)
    with _on(dev):
        _lib.check(_lib.lib().ao_qat_int4_fake_quantize(_ptr(w), _ptr(out), n, k, group_size, _stream()))
    return out


def qat_int4_fake_quantize_bwd(w: torch.Tensor, grad_out: torch.Tensor, group_size: int = 128) -> torch.Tensor:
    """The gradient autograd gives through the same lines (fake_quantizer.py:167-187): the straight-through term inside the clamp, plus
    the share of the group's maximum and minimum through the scale and the zero point (ties share it evenly).  w, grad_out bf16 [N, K]
    -> grad_w bf16 [N, K]; the range and the codes are made again from w."""
    name = "qat_int4_fake_quantize_bwd"
    dev, w, grad_out, n, k = _qat_int4_args(name, w, group_size, grad_out)
    grad_w = torch.empty_like(w)
    with _on(dev):
        _lib.check(_lib.lib().ao_qat_int4_fake_quantize_bwd(_ptr(w), _ptr(grad_out), _ptr(grad_w), n, k, group_size, _stream()))
    return grad_w


def _qat_fp8_args(name, x, hp_value_lb, hp_value_ub, grad_out=None):
    _qat_bf16(name, "x", x)
    if x.dim() < 1:
        raise RuntimeError(f"{name}: x must have at least one dimension")
    c = x.shape[-1]
    if c == 0 or c % 16 != 0:
        raise ValueError(f"{name}: C={c} must be a multiple of 16")
    lb = float("-inf") if hp_value_lb is None else float(hp_value_lb)
    ub = float("inf") if hp_value_ub is None else float(hp_value_ub)
    if not lb <= ub:
        raise ValueError(f"{name}: hp_value_lb={hp_value_lb} must not exceed hp_value_ub={hp_value_ub}")
    if grad_out is not None:
        _qat_bf16(name, "grad_out", grad_out)
        if grad_out.shape != x.shape:
            raise RuntimeError(f"{name}: grad_out has shape {tuple(grad_out.shape)} but x has {tuple(x.shape)}")
        grad_out = grad_out.contiguous()
    dev = _require_gpu(name, x, grad_out)
    x = x.contiguous()
    return dev, x, grad_out, x.numel() // c, c, lb, ub


def qat_fp8_fake_quantize_rowwise(x: torch.Tensor, hp_value_lb: Optional[float] = None, hp_value_ub: Optional[float] = None) -> torch.Tensor:
    """Float8FakeQuantizer.forward with PerRow() and float8_e4m3fn (fake_quantizer.py:84-98; quant_primitives.py:2173-2304): x bf16
    [..., C] -> bf16 [..., C], every row (all leading dimensions flattened) through scale = bf16(clamp(max|x|, lb, ub) / 448),
    q = e4m3(clamp(x / scale, -448, 448)), out = q scale.  A row whose clamped maximum is 0 comes back NaN, as in the reference."""
    name = "qat_fp8_fake_quantize_rowwise"
    dev, x, _, r, c, lb, ub = _qat_fp8_args(name, x, hp_value_lb, hp_value_ub)
    out = torch.empty_like(x)
    with _on(dev):
        _lib.check(_lib.lib().ao_qat_fp8_fake_quantize_rowwise(_ptr(x), _ptr(out), r, c, lb, ub, _stream()))
    return out


def qat_fp8_fake_quantize_rowwise_bwd(x: torch.Tensor, grad_out: torch.Tensor, hp_value_lb: Optional[float] = None,
                                      hp_value_ub: Optional[float] = None) -> torch.Tensor:
    """The gradient of that chain with every cast straight-through (the reference's own autograd rounds the incoming
    gradient to e4m3): the identity inside the +-448 clamp, plus the row maximum's share through the scale where the amax lies inside
    [lb, ub].  x, grad_out bf16 [..., C] -> grad_x bf16 [..., C]."""
    name = "qat_fp8_fake_quantize_rowwise_bwd"
    dev, x, grad_out, r, c, lb, ub = _qat_fp8_args(name, x, hp_value_lb, hp_value_ub, grad_out)
    grad_x = torch.empty_like(x)
    with _on(dev):
        _lib.check(_lib.lib().ao_qat_fp8_fake_quantize_rowwise_bwd(_ptr(x), _ptr(grad_out), _ptr(grad_x), r, c, lb, ub, _stream()))
    return grad_x


__all__ += ["qat_int4_fake_quantize", "qat_int4_fake_quantize_bwd", "qat_fp8_fake_quantize_rowwise", "qat_fp8_fake_quantize_rowwise_bwd"]


# ---- NF4 (QLoRA) weights: NF4Tensor's cast, dequantize and linear (include/ao_mi355.h "NF4") ---------------------------------
NF4_KERNELS = {0: "not fused", 1: "nf4_stream_kernel"}
NF4_BLOCK_SIZES = (32, 64, 128)


def _nf4_format(name, numel, block_size, scaler_block_size):
    """The sizes the kernels take, refused by reason before the library is touched."""
    if block_size not in NF4_BLOCK_SIZES:
        raise ValueError(f"{name}: block_size must be one of 32, 64, 128, got {block_size}")
    if not isinstance(scaler_block_size, int) or scaler_block_size < 1 or scaler_block_size & (scaler_block_size - 1):
        raise ValueError(f"{name}: scaler_block_size must be a power of two >= 1, got {scaler_block_size}")
    if numel % (block_size * scaler_block_size) != 0:
        raise ValueError(f"{name}: numel={numel} must be a multiple of block_size x scaler_block_size = {block_size} x {scaler_block_size}")
    if numel >= 1 << 31:
        raise ValueError(f"{name}: numel={numel} must be below 2^31")


def _nf4_bf16(name, what, t):
    if t.dtype != torch.bfloat16:
        raise RuntimeError(f"{name}: {what} must be bfloat16, got {t.dtype}")


def _nf4_mean(name, mean, dev):
    """scaler_mean as one bf16 on the device: read by the kernels through its pointer, never on the host."""
    if not isinstance(mean, torch.Tensor) or mean.numel() != 1 or mean.dtype != torch.bfloat16:
        raise RuntimeError(f"{name}: mean must be a bfloat16 tensor of one element")
    if mean.device != dev:
        raise RuntimeError(f"{name}: mean is on {mean.device}, the operands on {dev}")
    return mean.reshape(()).contiguous()


def _nf4_fields(name, codes, scalers, factors, block_size, scaler_block_size):
    """The three per-element / per-block fields of an NF4Tensor, flat and contiguous; returns them and numel."""
    if codes.dtype != torch.uint8 or codes.dim() != 1:
        raise RuntimeError(f"{name}: the codes must be a 1-D uint8 tensor [numel / 2], got {codes.dtype} {tuple(codes.shape)}")
    numel = codes.numel() * 2
    _nf4_format(name, numel, block_size, scaler_block_size)
    if scalers.dtype != torch.int8 or tuple(scalers.shape) != (numel // block_size,):
        raise RuntimeError(f"{name}: the scalers must be int8 [numel / block_size] = {(numel // block_size,)}, got {scalers.dtype} {tuple(scalers.shape)}")
    nsb = numel // (block_size * scaler_block_size)
    if factors.dtype != torch.bfloat16 or tuple(factors.shape) != (nsb,):
        raise RuntimeError(f"{name}: the factors must be bfloat16 [numel / (block_size x scaler_block_size)] = {(nsb,)}, got {factors.dtype} "
                           f"{tuple(factors.shape)}")
    return codes.contiguous(), scalers.contiguous(), factors.contiguous(), numel


def nf4_block_absmax(x: torch.Tensor, block_size: int = 64) -> torch.Tensor:
    """get_block_absmax (nf4_tensor.py:560-577) on the flattened tensor: x bf16, any shape -> bf16 [numel / block_size]."""
    name = "nf4_block_absmax"
    _nf4_bf16(name, "x", x)
    _nf4_format(name, x.numel(), block_size, 1)
    dev = _require_gpu(name, x)
    x = x.contiguous()
    out = torch.empty((x.numel() // block_size,), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nf4_block_absmax(_ptr(x), _ptr(out), x.numel(), block_size, _stream()))
    return out


def nf4_quantize(x: torch.Tensor, absmax: torch.Tensor, mean: torch.Tensor, block_size: int = 64, scaler_block_size: int = 256):
    """The rest of NF4Tensor.from_tensor (nf4_tensor.py:649-718) in one launch, the reference's bytes: x bf16 (any shape, flattened),
    absmax = nf4_block_absmax(x), mean = absmax.mean() (torch's, on the device) -> (quantized_data uint8 [numel / 2], quantized_scalers
    int8 [numel / block_size], quantization_factor bf16 [numel / (block_size x scaler_block_size)])."""
    name = "nf4_quantize"
    _nf4_bf16(name, "x", x)
    _nf4_bf16(name, "absmax", absmax)
    numel = x.numel()
    _nf4_format(name, numel, block_size, scaler_block_size)
    if tuple(absmax.shape) != (numel // block_size,):
        raise RuntimeError(f"{name}: absmax must be [numel / block_size] = {(numel // block_size,)}, got {tuple(absmax.shape)}")
    dev = _require_gpu(name, x, absmax, mean)
    mean = _nf4_mean(name, mean, dev)
    x, absmax = x.contiguous(), absmax.contiguous()
    codes = torch.empty((numel // 2,), dtype=torch.uint8, device=dev)
    scalers = torch.empty((numel // block_size,), dtype=torch.int8, device=dev)
    factors = torch.empty((numel // (block_size * scaler_block_size),), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nf4_quantize(_ptr(x), _ptr(absmax), _ptr(mean), _ptr(codes), _ptr(scalers), _ptr(factors), numel, block_size,
                                              scaler_block_size, _stream()))
    return codes, scalers, factors


def nf4_dequantize(codes, scalers, factors, mean, block_size: int = 64, scaler_block_size: int = 256) -> torch.Tensor:
    """NF4Tensor.get_original_weight (nf4_tensor.py:845-871) in one launch, flat: -> bf16 [numel] (the caller views it as the weight)."""
    name = "nf4_dequantize"
    codes, scalers, factors, numel = _nf4_fields(name, codes, scalers, factors, block_size, scaler_block_size)
    dev = _require_gpu(name, codes, scalers, factors, mean)
    mean = _nf4_mean(name, mean, dev)
    w = torch.empty((numel,), dtype=torch.bfloat16, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_nf4_dequantize(_ptr(codes), _ptr(scalers), _ptr(factors), _ptr(mean), _ptr(w), numel, block_size, scaler_block_size,
                                                _stream()))
    return w


def nf4_linear_route(m: int, n: int, k: int, block_size: int = 64, scaler_block_size: int = 256) -> dict:
    """The route nf4_linear takes for a shape (host logic only, ao_nf4_linear_route): kernel "nf4_stream_kernel", or "not fused" --
    dequantize, then multiply -- above the seam and for shapes the kernel does not take (K % block_size != 0)."""
    return _two_form_route("ao_nf4_linear_route", NF4_KERNELS, m, n, k, block_size, scaler_block_size)


def nf4_linear_kernel_name(m: int, n: int, k: int, block_size: int = 64, scaler_block_size: int = 256) -> str:
    return _two_form_kernel_name("ao_nf4_linear_kernel_name", m, n, k, block_size, scaler_block_size)


def nf4_set_form(form: int) -> None:
    """Measurement only: 0 the product route, 1 the stream kernel at any M (calling thread).  There is no tiled form."""
    _two_form_set_form("ao_nf4_linear_set_form", form)


def nf4_linear(x2, codes, scalers, factors, mean, n: int, k: int, block_size: int = 64, scaler_block_size: int = 256, out=None):
    """LinearNF4.forward (nf4_tensor.py:1053-1058) on a 2-D bf16 activation: bf16(x . w^T) with w [n, k] the bits of nf4_dequantize, fp32
    accumulation, no bias.  By the route: one launch that streams the fields once, or nf4_dequantize + F.linear."""
    name = "nf4_linear"
    if x2.dim() != 2 or x2.dtype != torch.bfloat16:
        raise RuntimeError(f"{name}: x must be a 2-D bfloat16 tensor, got {tuple(x2.shape)} {x2.dtype}")
    codes, scalers, factors, numel = _nf4_fields(name, codes, scalers, factors, block_size, scaler_block_size)
    if n < 1 or k < 1 or n * k != numel:
        raise RuntimeError(f"{name}: the weight shape [{n}, {k}] does not hold the {numel} elements of the fields")
    m, kx = x2.shape
    if kx != k:
        raise RuntimeError(f"{name}: K mismatch {kx} vs {k}")
    dev = _require_gpu(name, x2, codes, scalers, factors, mean)
    mean = _nf4_mean(name, mean, dev)
    x2 = x2.contiguous()
    if nf4_linear_route(m, n, k, block_size, scaler_block_size)["kernel"] != NF4_KERNELS[1]:
        w = nf4_dequantize(codes, scalers, factors, mean, block_size, scaler_block_size).view(n, k)
        y = torch.nn.functional.linear(x2, w)
        return y if out is None else _bf16_out(name, out, m, n, dev).copy_(y)
    y = _bf16_out(name, out, m, n, dev)
    if m > 0:
        with _on(dev):
            _lib.check(_lib.lib().ao_nf4_linear(_ptr(x2), _ptr(codes), _ptr(scalers), _ptr(factors), _ptr(mean), _ptr(y), m, n, k, block_size,
                                                scaler_block_size, _stream()))
    return y


__all__ += ["nf4_block_absmax", "nf4_quantize", "nf4_dequantize", "nf4_linear", "nf4_linear_route", "nf4_linear_kernel_name", "nf4_set_form"]


# ---- low-bit optimizers: torchao/optim's state casts and its Adam step (include/ao_mi355.h "Low-bit optimizers") ---------------
OPTIM_FORMATS = {"Q8_SIGNED": 0, "Q8_UNSIGNED": 1, "Q4_SIGNED": 2, "Q4_UNSIGNED": 3, "FP8": 4, "PLAIN": 5}
OPTIM_BLOCK_SIZES = (64, 128, 256, 512, 1024, 2048)
OPTIM_SCALARS = ("lr", "lr_wd", "wd", "one_minus_beta1", "one_minus_beta2", "bias_correction1", "sqrt_bias_correction2", "eps")
_OPTIM_Q8, _OPTIM_Q4, _OPTIM_FP8, _OPTIM_PLAIN = (0, 1), (2, 3), (4,), (5,)


def _optim_format(name, fmt, n, block_size, allowed):
    """The formats and sizes the kernels take, refused by reason before the library is touched."""
    if fmt not in allowed:
        names = ", ".join(k for k, v in OPTIM_FORMATS.items() if v in allowed)
        raise ValueError(f"{name}: format must be one of {names}, got {fmt}")
    if fmt in _OPTIM_PLAIN:
        return
    if block_size not in OPTIM_BLOCK_SIZES:
        raise ValueError(f"{name}: block_size must be a power of two from 64 to 2048, got {block_size}")
    if n % block_size != 0:
        raise ValueError(f"{name}: numel={n} must be a multiple of block_size={block_size}")


def _optim_fields(name, what, codes, scale, qmap, fmt, n, block_size, dev):
    """One quantized state's fields against its format: contiguous codes (as bytes), fp32 scale [n / block_size], the state's own table."""
    want = n // 2 if fmt in _OPTIM_Q4 else n
    ok_dtype = (torch.float8_e4m3fn, torch.uint8) if fmt in _OPTIM_FP8 else (torch.uint8,)
    if codes.dtype not in ok_dtype or codes.numel() != want or not codes.is_contiguous():
        raise RuntimeError(f"{name}: {what} codes must be contiguous {ok_dtype[0]} with {want} elements, got {codes.dtype} {tuple(codes.shape)}")
    if scale is None or scale.dtype != torch.float32 or tuple(scale.shape) != (n // block_size,) or not scale.is_contiguous():
        raise RuntimeError(f"{name}: {what} scale must be contiguous float32 [numel / block_size] = {(n // block_size,)}")
    if fmt in _OPTIM_FP8:
        if qmap is not None:
            raise RuntimeError(f"{name}: the FP8 format has no qmap")
    else:
        entries = 16 if fmt in _OPTIM_Q4 else 256
        if qmap is None or qmap.dtype != torch.float32 or tuple(qmap.shape) != (entries,) or not qmap.is_contiguous():
            raise RuntimeError(f"{name}: {what} qmap must be contiguous float32 [{entries}]")
    for t in (codes, scale, qmap):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name}: {what} fields are on {t.device}, the operands on {dev}")


def optim_grid(n: int, max_workgroups: int = 0) -> dict:
    """The grid rule of the optimizer kernels (ao_optim_grid, host logic only): elements a workgroup takes per trip of its loop, trips in
    all, workgroups launched."""
    out = (ctypes.c_int64 * 3)()
    _lib.check(_lib.lib().ao_optim_grid(int(n), int(max_workgroups), out))
    return {"tile": out[0], "tiles": out[1], "workgroups": out[2]}


def optim_quantize(src: torch.Tensor, format: int, block_size: int, qmap: Optional[torch.Tensor] = None, codes=None, scale=None):
    """The subclasses' copy_ from a float tensor (subclass_8bit.py:137-141, subclass_4bit.py:155-159, subclass_fp8.py:115-118) in one
    launch, the reference's bytes: src fp32 or bf16 (any shape, taken flat) -> (codes, scale); written into `codes` / `scale` when given."""
    name = "optim_quantize"
    if src.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"{name}: src must be float32 or bfloat16, got {src.dtype}")
    n = src.numel()
    _optim_format(name, format, n, block_size, _OPTIM_Q8 + _OPTIM_Q4 + _OPTIM_FP8)
    dev = _require_gpu(name, src, qmap, codes, scale)
    src = src.contiguous()
    if codes is None:
        codes = torch.empty((n // 2,) if format in _OPTIM_Q4 else tuple(src.shape), dtype=torch.float8_e4m3fn if format in _OPTIM_FP8 else torch.uint8,
                            device=dev)
    if scale is None:
        scale = torch.empty((n // block_size,), dtype=torch.float32, device=dev)
    _optim_fields(name, "the", codes, scale, qmap, format, n, block_size, dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_optim_quantize(_ptr(src), int(src.dtype == torch.bfloat16), _ptr(codes), _ptr(scale), _ptr(qmap), n, block_size,
                                                format, _stream()))
    return codes, scale


def optim_dequantize(codes, scale, format: int, block_size: int, qmap: Optional[torch.Tensor] = None, dtype=torch.float32) -> torch.Tensor:
    """dequantize() of the three state subclasses in one launch, flat: -> fp32 [numel] (or that rounded to bf16)."""
    name = "optim_dequantize"
    if dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"{name}: dtype must be float32 or bfloat16, got {dtype}")
    n = codes.numel() * (2 if format in _OPTIM_Q4 else 1)
    _optim_format(name, format, n, block_size, _OPTIM_Q8 + _OPTIM_Q4 + _OPTIM_FP8)
    dev = _require_gpu(name, codes, scale, qmap)
    _optim_fields(name, "the", codes, scale, qmap, format, n, block_size, dev)
    out = torch.empty((n,), dtype=dtype, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ao_optim_dequantize(_ptr(codes), _ptr(scale), _ptr(qmap), _ptr(out), int(dtype == torch.bfloat16), n, block_size,
                                                  format, _stream()))
    return out


def optim_adam_step(p, grad, m_codes, m_scale, m_qmap, v_codes, v_scale, v_qmap, vmax_codes, vmax_scale, vmax_qmap, format: int,
                    block_size: int, scalars, is_adamw: bool, sr: bool = False, seed: int = 0, step: int = 0, param_index: int = 0,
                    max_workgroups: int = 0) -> None:
    """single_param_adam (torchao/optim/adam.py:163-209) for one parameter in ONE launch, the bytes of the reference's eager CPU run: p (bf16
    or fp32, contiguous) and the moments' codes and scales are updated in place.  format: Q8_SIGNED / Q4_SIGNED / FP8 (the first moment's),
    or PLAIN, where m_codes / v_codes / vmax_codes are the moments themselves in p's dtype.  vmax_codes None: no amsgrad.  scalars: the eight
    fp32 values of OPTIM_SCALARS for this step (ao_amd.optim.adam.step_scalars).  sr: stochastic rounding of a bf16 p from (seed, step,
    param_index, element).  max_workgroups caps the grid (0: the default); the bytes do not depend on it."""
    name = "optim_adam_step"
    if p.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"{name}: p must be float32 or bfloat16, got {p.dtype}")
    if grad.dtype != p.dtype:
        raise RuntimeError(f"{name}: grad must have p's dtype {p.dtype}, got {grad.dtype}")
    if grad.shape != p.shape:
        raise RuntimeError(f"{name}: grad {tuple(grad.shape)} must have p's shape {tuple(p.shape)}")
    if not p.is_contiguous():
        raise RuntimeError(f"{name}: p is updated in place and must be contiguous")
    if sr and p.dtype != torch.bfloat16:
        raise RuntimeError(f"{name}: stochastic rounding is for bfloat16 parameters, got {p.dtype}")
    if len(scalars) != len(OPTIM_SCALARS):
        raise ValueError(f"{name}: scalars must hold {len(OPTIM_SCALARS)} values ({', '.join(OPTIM_SCALARS)}), got {len(scalars)}")
    n = p.numel()
    _optim_format(name, format, n, block_size, (0, 2, 4, 5))
    dev = _require_gpu(name, p, grad, m_codes, v_codes, vmax_codes)
    grad = grad.contiguous()
    states = [("exp_avg", m_codes, m_scale, m_qmap, format), ("exp_avg_sq", v_codes, v_scale, v_qmap, format + (1 if format in (0, 2) else 0))]
    if vmax_codes is not None:
        states.append(("max_exp_avg_sq", vmax_codes, vmax_scale, vmax_qmap, states[1][4]))
    for what, codes, scale, qmap, fmt in states:
        if format in _OPTIM_PLAIN:
            if codes.dtype != p.dtype or codes.numel() != n or not codes.is_contiguous() or codes.device != dev:
                raise RuntimeError(f"{name}: a plain {what} must be contiguous {p.dtype} with p's {n} elements on {dev}")
            if scale is not None or qmap is not None:
                raise RuntimeError(f"{name}: a plain {what} has no scale and no qmap")
        else:
            _optim_fields(name, what, codes, scale, qmap, fmt, n, block_size, dev)
    s = _lib.OptimScalars(*[float(x) for x in scalars])
    seed = int(seed) & (2 ** 64 - 1)  # torch.initial_seed() is unsigned; the entry takes the same 64 bits as an int64
    seed -= 2 ** 64 if seed >= 2 ** 63 else 0
    with _on(dev):
        _lib.check(_lib.lib().ao_optim_adam_step(
            _ptr(p), _ptr(grad), int(p.dtype == torch.bfloat16), _ptr(m_codes), _ptr(m_scale), _ptr(m_qmap), _ptr(v_codes), _ptr(v_scale),
            _ptr(v_qmap), _ptr(vmax_codes), _ptr(vmax_scale), _ptr(vmax_qmap), format, n, block_size if format not in _OPTIM_PLAIN else 0,
            ctypes.byref(s), int(bool(is_adamw)), int(bool(sr)), int(seed), int(step), int(param_index), int(max_workgroups), _stream()))


__all__ += ["optim_grid", "optim_quantize", "optim_dequantize", "optim_adam_step", "OPTIM_FORMATS", "OPTIM_BLOCK_SIZES", "OPTIM_SCALARS"]


# ---------------------------------------------------------------------------
# GPTQ: one block of the column loop in one launch
# ---------------------------------------------------------------------------
GPTQ_INT4, GPTQ_INT8, GPTQ_NVFP4 = 0, 1, 2
GPTQ_MAX_BLOCK = 256


def gptq_block(W: torch.Tensor, Hinv: torch.Tensor, k0: int, block_cols: int, format: int, qdata: torch.Tensor, *, group_size: int = 0,
               scale: Optional[torch.Tensor] = None, zero_point: Optional[torch.Tensor] = None, row_scale: Optional[torch.Tensor] = None,
               per_tensor_scale: Optional[torch.Tensor] = None, err: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The column loop of gptq_quantize (prototype/gptq/api.py:446-532) over the GPTQ block of columns [k0, k0 + block_cols), and the final
    codes of those columns (:537-569), in one launch (csrc/gptq_kernels.hip states the arithmetic).  In place: W (bf16 or fp32 [N, K],
    contiguous) is updated in the block's columns; the block's part of the outputs is written -- qdata (GPTQ_INT4 / GPTQ_NVFP4: uint8
    [N, K/2], even k in the low nibble; GPTQ_INT8: int8 [N, K]), GPTQ_INT4: scale / zero_point [K/g, N] in W's dtype, GPTQ_NVFP4: scale
    float8_e4m3fn [N, K/16] under per_tensor_scale (one fp32 on the device), GPTQ_INT8: under row_scale (fp32 [N], given).  Hinv: fp32
    [K, K], the upper Cholesky factor of the inverse Hessian.  Returns Err, fp32 [N, block_cols]: what the lazy batch update multiplies."""
    name = "gptq_block"
    dev = _require_gpu(name, W, Hinv, qdata, scale, zero_point, row_scale, per_tensor_scale, err)
    if W.dtype not in (torch.bfloat16, torch.float32):
        raise NotImplementedError(f"{name}: weights are bfloat16 or float32, got {W.dtype}")
    if W.dim() != 2 or not W.is_contiguous():
        raise RuntimeError(f"{name}: W must be a contiguous 2-D tensor (it is updated in place)")
    n, k = W.shape
    if Hinv.dtype != torch.float32 or tuple(Hinv.shape) != (k, k) or not Hinv.is_contiguous():
        raise RuntimeError(f"{name}: Hinv must be a contiguous float32 [{k}, {k}] tensor")
    if block_cols > GPTQ_MAX_BLOCK:
        raise ValueError(f"{name}: a GPTQ block holds at most {GPTQ_MAX_BLOCK} columns (its tile of W and Err stay in LDS), got {block_cols}")

    def field(what, t, dtypes, shape):
        if t is None or t.dtype not in dtypes or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"{name}: {what} must be a contiguous {' / '.join(str(d) for d in dtypes)} tensor of shape {shape}")
        return t

    aux = None
    if format == GPTQ_INT4:
        field("qdata", qdata, (torch.uint8,), (n, k // 2))
        if group_size <= 0 or k % group_size != 0:
            raise ValueError(f"{name}: group_size {group_size} must divide K={k}")
        field("scale", scale, (W.dtype,), (k // group_size, n))
        field("zero_point", zero_point, (W.dtype,), (k // group_size, n))
    elif format == GPTQ_NVFP4:
        group_size = 16
        field("qdata", qdata, (torch.uint8,), (n, k // 2))
        field("scale", scale, (torch.float8_e4m3fn, torch.uint8), (n, k // 16))
        aux = _nvfp4_scalar(name, "per_tensor_scale", per_tensor_scale, dev)
        if aux is None:
            raise RuntimeError(f"{name}: NVFP4 needs the per-tensor scale")
    elif format == GPTQ_INT8:
        field("qdata", qdata, (torch.int8,), (n, k))
        aux = field("row_scale", None if row_scale is None else row_scale.reshape(-1), (torch.float32,), (n,))
    else:
        raise ValueError(f"{name}: unknown format {format}")
    if err is None:
        err = torch.empty((n, block_cols), dtype=torch.float32, device=dev)
    else:
        field("err", err, (torch.float32,), (n, block_cols))
    with _on(dev):
        _lib.check(_lib.lib().ao_gptq_block(_ptr(W), int(W.dtype == torch.bfloat16), _ptr(Hinv), _ptr(err), format, group_size, _ptr(qdata),
                                            _ptr(scale), _ptr(zero_point), _ptr(aux), n, k, int(k0), int(block_cols), _stream()))
    return err


__all__ += ["gptq_block", "GPTQ_INT4", "GPTQ_INT8", "GPTQ_NVFP4", "GPTQ_MAX_BLOCK"]


# ---------------------------------------------------------------------------
# AWQ: the error matrices of R candidate scale vectors in one launch
# ---------------------------------------------------------------------------
AWQ_GROUP_SIZES = (32, 64, 128, 256)


def awq_scaled_error(W: torch.Tensor, S: torch.Tensor, group_size: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The weight's side of AWQObserver.calculate_qparams' search (prototype/awq/core.py:70-86) for the R candidate scale vectors S at
    once (csrc/awq_kernels.hip states the arithmetic).  W bf16 [N, K]; S bf16 [R, K], finite and positive; returns D fp32 [R, N, K] with
    D[r] = W - Int4Tensor.from_hp(W * S[r], [1, group_size]).dequantize() / S[r], every step one fp32 operation rounded once, so that the
    reference's loss of ratio r is tr(D[r] G D[r]^T) / (rows N) with G = X^T X.  out: an exact-size contiguous fp32 buffer to write into."""
    name = "awq_scaled_error"
    dev = _require_gpu(name, W, S, out)
    if W.dtype != torch.bfloat16 or S.dtype != torch.bfloat16:
        raise NotImplementedError(f"{name}: W and S are bfloat16, got {W.dtype} and {S.dtype}")
    if W.dim() != 2 or not W.is_contiguous():
        raise RuntimeError(f"{name}: W must be a contiguous 2-D tensor [N, K], got shape {tuple(W.shape)}")
    n, k = W.shape
    if S.dim() != 2 or S.shape[1] != k or not S.is_contiguous():
        raise RuntimeError(f"{name}: S must be a contiguous [R, {k}] tensor, got shape {tuple(S.shape)}")
    r = S.shape[0]
    if group_size not in AWQ_GROUP_SIZES:
        raise ValueError(f"{name}: group_size must be one of 32, 64, 128, 256, got {group_size}")
    if k == 0 or k % group_size != 0:
        raise ValueError(f"{name}: K={k} must be a multiple of group_size={group_size}")
    if out is None:
        out = torch.empty((r, n, k), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (r, n, k) or not out.is_contiguous():
        raise RuntimeError(f"{name}: out must be a contiguous float32 tensor of shape {(r, n, k)}")
    with _on(dev):
        _lib.check(_lib.lib().ao_awq_scaled_error(_ptr(W), _ptr(S), _ptr(out), n, k, r, group_size, _stream()))
    return out


__all__ += ["awq_scaled_error", "AWQ_GROUP_SIZES"]


# ---------------------------------------------------------------------------
# SmoothQuant: the calibration reductions, and the int8 activation casts with the activation pre-scale folded in
# (csrc/smoothquant_kernels.hip states the reductions' arithmetic, csrc/quant_kernels.hip the casts')
# ---------------------------------------------------------------------------
def _sq_rows(name, x):
    if x.dtype != torch.bfloat16:
        raise NotImplementedError(f"{name}: x is bfloat16, got {x.dtype}")
    if x.dim() != 2:
        raise RuntimeError(f"{name}: expected a 2-D tensor, got {x.dim()}-D")
    if x.shape[1] == 0 or x.shape[1] % 8 != 0:
        raise ValueError(f"{name}: K={x.shape[1]} must be a multiple of 8")
    return x if x.is_contiguous() else x.contiguous()


def _sq_vector(name, what, v, k):
    """A bf16 [K] vector (the smoothing factor or the activation pre-scale), contiguous."""
    if v.dtype != torch.bfloat16 or v.numel() != k:
        raise RuntimeError(f"{name}: {what} must be a bfloat16 vector of K = {k} elements, got {v.dtype} {tuple(v.shape)}")
    return v.reshape(-1).contiguous()


def sq_col_absmax_update(x: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """state[k] = max(state[k], max_m |x[m, k]|) in place (SmoothQuantObserver's x_abs_max, prototype/smoothquant/core.py:53, as a running
    maximum).  x bf16 [M, K]; state fp32 [K], contiguous, non-negative (zeros before the first update).  Exact and order-independent."""
    name = "sq_col_absmax_update"
    dev = _require_gpu(name, x, state)
    x = _sq_rows(name, x)
    m, k = x.shape
    if state.dtype != torch.float32 or tuple(state.shape) != (k,) or not state.is_contiguous():
        raise RuntimeError(f"{name}: state must be a contiguous float32 vector of K = {k} elements, got {state.dtype} {tuple(state.shape)}")
    with _on(dev):
        _lib.check(_lib.lib().ao_sq_col_absmax_update(_ptr(x), _ptr(state), m, k, _stream()))
    return state


def sq_smoothed_amax_update(x: torch.Tensor, s: torch.Tensor, amax: torch.Tensor) -> torch.Tensor:
    """amax = max(amax, max |bf16(x / s)|) in place: the amax of the smoothed activation `x / smoothing_factor` (core.py:66-68, 192-195)
    without writing it.  x bf16 [M, K]; s bf16 [K]; amax fp32, one element, non-negative."""
    name = "sq_smoothed_amax_update"
    dev = _require_gpu(name, x, s, amax)
    x = _sq_rows(name, x)
    m, k = x.shape
    s = _sq_vector(name, "s", s, k)
    if amax.dtype != torch.float32 or amax.numel() != 1:
        raise RuntimeError(f"{name}: amax must be a float32 tensor of one element, got {amax.dtype} {tuple(amax.shape)}")
    with _on(dev):
        _lib.check(_lib.lib().ao_sq_smoothed_amax_update(_ptr(x), _ptr(s), _ptr(amax), m, k, _stream()))
    return amax


def int8_quantize_rowwise_prescaled(x: torch.Tensor, pre: torch.Tensor):
    """int8_quantize_rowwise(x * pre) in one launch, the product never written: x bf16 [M, K], pre bf16 [K] ->
    (qdata int8 [M, K], scale fp32 [M, 1])."""
    return _int8_quantize_rowwise("int8_quantize_rowwise_prescaled", x, pre)


def _int8_quantize_tensorwise_prescaled_rows(x, pre):
    """(qdata int8 [M, K], scale fp32 [M] with the tensor's scale in every entry: what the GEMM's row-scale operand takes as it is)"""
    name = "int8_quantize_tensorwise_prescaled"
    dev = _require_gpu(name, x, pre)
    x = _sq_rows(name, x)
    m, k = x.shape
    pre = _sq_vector(name, "pre", pre, k)
    q = torch.empty((m, k), dtype=torch.int8, device=dev)
    s = torch.empty((m + 1,), dtype=torch.float32, device=dev)  # the last entry is the call's amax work buffer
    with _on(dev):
        _lib.check(_lib.lib().ao_int8_quantize_tensorwise_prescaled(_ptr(x), _ptr(pre), _ptr(s[m:]), _ptr(q), _ptr(s), m, k, _stream()))
    return q, s[:m]


def int8_quantize_tensorwise_prescaled(x: torch.Tensor, pre: torch.Tensor):
    """int8_quantize_tensorwise(x * pre) without writing the product: x bf16 [M, K], pre bf16 [K] -> (qdata int8 [M, K], scale fp32 [1, 1])."""
    q, s = _int8_quantize_tensorwise_prescaled_rows(x, pre)
    return q, s[:1].reshape(1, 1)


def int8_quantize_static_prescaled(x: torch.Tensor, pre: torch.Tensor, scale: torch.Tensor, zero_point: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int8_quantize_static(x * pre, scale, zero_point) in one launch: x bf16 [M, K], pre bf16 [K], scale fp32 of 1 or M elements (and an int8
    zero-point of the same shape, or None) -> qdata int8 [M, K]."""
    return _int8_quantize_static("int8_quantize_static_prescaled", x, scale, zero_point, pre)


def int8_linear_prescaled(x2, pre, wq, w_scale, bias=None):
    """int8_linear(x2 * pre, ...) for an Int8Tensor with a per-input-feature act_pre_scale (SmoothQuant): the pre-scaled cast, then
    ao_int8_scaled_mm.  Same bits as the multiply followed by int8_linear.  (The Int8Tensor linear does not come here with one row: there
    the multiply and the one-launch fused cast + matmul kernel stay)"""
    xq, xs = int8_quantize_rowwise_prescaled(x2, pre)
    return int8_scaled_mm(xq, xs, wq, w_scale, bias)


def int8_linear_tensorwise_prescaled(x2, pre, wq, w_scale, bias=None):
    """int8_linear_tensorwise(x2 * pre, ...) without writing the product."""
    xq, xs = _int8_quantize_tensorwise_prescaled_rows(x2, pre)
    return int8_scaled_mm(xq, xs, wq, w_scale, bias)


def int8_linear_static_prescaled(x2, pre, wq, w_scale, act_scale, act_zero_point=None, w_row_sums=None, bias=None):
    """int8_linear_static(x2 * pre, ...) without writing the product."""
    m = x2.shape[0]
    xq = int8_quantize_static_prescaled(x2, pre, act_scale, act_zero_point)
    return _int8_linear_static(xq, m, wq, w_scale, act_scale, act_zero_point, w_row_sums, bias)


__all__ += ["sq_col_absmax_update", "sq_smoothed_amax_update", "int8_quantize_rowwise_prescaled", "int8_quantize_tensorwise_prescaled",
            "int8_quantize_static_prescaled", "int8_linear_prescaled", "int8_linear_tensorwise_prescaled", "int8_linear_static_prescaled"]
