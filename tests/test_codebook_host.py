"""Codebook weights without a GPU: the config and its registration, each named refusal, the C entries' argument checks, the route."""
import ctypes

import pytest
import torch

from ao_amd import _lib, ops
from ao_amd.prototype import (CodebookQuantizedTensor, CodebookWeightOnlyConfig, choose_qparams_codebook, codebook_weight_only,
                              dequantize_codebook, quantize_codebook)
from ao_amd.quantization import quantize_
from ao_amd.quantization.quant_api import _QUANTIZE_CONFIG_HANDLER

SEAM = 64


def test_config_defaults_and_registration():
    c = CodebookWeightOnlyConfig()
    assert (c.dtype, c.block_size, c.scale_block_size) == (torch.uint4, (1, 1), None)
    assert codebook_weight_only is CodebookWeightOnlyConfig and CodebookWeightOnlyConfig in _QUANTIZE_CONFIG_HANDLER
    for name in ("codebook_assign", "codebook_lloyd_step", "codebook_dequantize", "codebook_linear", "codebook_linear_route"):
        assert name in ops.__all__


def _w(n=16, k=64, dtype=torch.bfloat16):
    return torch.zeros(n, k, dtype=dtype)


@pytest.mark.parametrize("w,block,dtype,sb,exc,word", [
    (_w(), (1, 1), torch.uint3, 64, NotImplementedError, "torch.uint3 is not built"),
    (_w(), (1, 1), torch.uint7, 64, NotImplementedError, "use torch.uint4"),
    (_w(), (1, 1), torch.int32, 64, NotImplementedError, "65536-entry table"),
    (_w(), (2, 4), torch.uint8, 64, NotImplementedError, r"block_size \(2, 4\) is not built"),
    (_w(), (1, 16), torch.uint8, 64, NotImplementedError, r"block_size \(1, 16\) is not built"),
    (_w(dtype=torch.float32), (1, 1), torch.uint8, 64, NotImplementedError, "float16 and float32 are not built"),
    (_w(dtype=torch.float16), (1, 4), torch.uint8, 64, NotImplementedError, "float16 and float32 are not built"),
    (torch.zeros(4, 4, 64, dtype=torch.bfloat16), (1, 1), torch.uint8, 64, NotImplementedError, "expected a 2-D weight"),
    (_w(), (1, 4), torch.uint8, 48, ValueError, r"must be divisible by scale_block_size \(48\)"),
    (_w(k=72), (1, 8), torch.uint8, 36, ValueError, r"scale_block_size \(36\) must be a multiple of the block width 8"),
    (_w(k=40), (1, 8), torch.uint4, 40, ValueError, "K / d = 5 must be even for torch.uint4"),
    (_w(), (1, 4), torch.uint8, 64, RuntimeError, "no CPU fallback"),
])
def test_named_refusals_before_any_launch(w, block, dtype, sb, exc, word):
    with pytest.raises(exc, match=word):
        CodebookQuantizedTensor.from_float(w, block, dtype, sb)


def test_handler_ops_and_tensor_refusals():
    with pytest.raises(NotImplementedError, match="devices= .* is not built"):
        choose_qparams_codebook(_w(), (1, 1), 64, torch.uint8, devices=[torch.device("cpu")])
    with pytest.raises(NotImplementedError, match="torch.uint2 is not built"):
        quantize_(torch.nn.Linear(64, 16, dtype=torch.bfloat16), CodebookWeightOnlyConfig(dtype=torch.uint2))
    with pytest.raises(NotImplementedError, match="torch.uint5 is not built"):
        quantize_codebook(_w(), torch.zeros(32, 1, 1), torch.ones(16, 1, 1), code_dtype=torch.uint5)
    t = CodebookQuantizedTensor(torch.zeros(16, 32, dtype=torch.uint8), torch.zeros(16, 1, 1, dtype=torch.bfloat16), (1, 1),
                                torch.ones(16, 1, 1, dtype=torch.bfloat16), (16, 64), dtype=torch.bfloat16)
    assert t.shape == (16, 64) and t.dtype == torch.bfloat16 and isinstance(t.detach(), CodebookQuantizedTensor)
    p = torch.nn.Parameter(t, requires_grad=False)
    assert type(p) is CodebookQuantizedTensor and not p.requires_grad
    with pytest.raises(NotImplementedError, match="activations must be bfloat16"):
        torch.nn.functional.linear(torch.zeros(2, 64), p)
    for call in (lambda: torch.nn.functional.linear(torch.zeros(2, 64, dtype=torch.bfloat16), p), t.dequantize,
                 lambda: dequantize_codebook(t.codes, t.codebook, t.scales)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    inner, ctx = t.__tensor_flatten__()
    back = CodebookQuantizedTensor.__tensor_unflatten__({n: getattr(t, n) for n in inner}, ctx, None, None)
    assert back.shape == t.shape and back.block_size == (1, 1) and back.codes is t.codes


def test_weights_above_2_to_27_elements_are_left_untouched():
    lin = torch.nn.Linear(2 ** 14, 2 ** 13 + 1, bias=False, dtype=torch.bfloat16, device="meta")
    weight = lin.weight
    quantize_(lin, CodebookWeightOnlyConfig(dtype=torch.uint8))
    assert lin.weight is weight and type(lin.weight) is torch.nn.Parameter


def test_abi_refuses_shapes_then_null_pointers():
    lib, declared = _lib.lib(), _lib.declared_symbols()
    names = ["ao_codebook_assign", "ao_codebook_lloyd_workspace_bytes", "ao_codebook_lloyd_step", "ao_codebook_pack_u4", "ao_codebook_dequantize",
             "ao_codebook_linear_fits", "ao_codebook_linear_route", "ao_codebook_linear_kernel_name", "ao_codebook_linear_set_form", "ao_codebook_linear"]
    for name in names:
        assert hasattr(lib, name) and name in declared and name in _lib._SIGNATURES
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    calls = [
        (lambda: lib.ao_codebook_assign(one, one, one, 4, 3, 256, None), "d must be 1, 2, 4 or 8"),
        (lambda: lib.ao_codebook_assign(one, one, one, 4, 4, 64, None), "k must be 16"),
        (lambda: lib.ao_codebook_lloyd_step(one, one, one, one, None, one, 0, 4, 8, 256, None), "the workspace holds 0 bytes"),
        (lambda: lib.ao_codebook_pack_u4(one, one, 5, None), "n=5 must be even"),
        (lambda: lib.ao_codebook_dequantize(one, one, one, one, 4, 64, 4, 256, 48, None), "sb must divide K"),
        (lambda: lib.ao_codebook_dequantize(one, one, one, one, 4, 64, 8, 256, 4, None), "multiple of d"),
        (lambda: lib.ao_codebook_dequantize(one, one, one, one, 4, 40, 8, 16, 40, None), "K / d must be even"),
        (lambda: lib.ao_codebook_linear(one, one, one, one, one, 4, 16, 48, 4, 256, 48, None), "multiples of 32"),
        (lambda: lib.ao_codebook_linear(one, one, one, one, one, SEAM + 1, 16, 64, 4, 256, 64, None), "is not fused"),
        (lambda: lib.ao_codebook_linear_set_form(2), "there is no tiled form"),
    ]
    for call, word in calls:
        assert call() == _lib.AO_ERR_INVALID_ARGUMENT and word in _lib.last_error(), (word, _lib.last_error())
    ws = lib.ao_codebook_lloyd_workspace_bytes(4, 8, 256)
    assert ws == 256 * 9 * 4 and lib.ao_codebook_lloyd_workspace_bytes(4, 3, 256) == -1
    for call in (lambda: lib.ao_codebook_assign(None, one, one, 4, 8, 256, None), lambda: lib.ao_codebook_lloyd_step(one, one, None, one, None, one, ws, 4, 8, 256, None),
                 lambda: lib.ao_codebook_pack_u4(None, one, 4, None), lambda: lib.ao_codebook_dequantize(one, None, one, one, 4, 64, 4, 256, 32, None),
                 lambda: lib.ao_codebook_linear(None, one, one, one, one, 4, 16, 64, 4, 256, 64, None)):
        assert call() == _lib.AO_ERR_NULL_POINTER and "null pointer" in _lib.last_error()
    for call in (lambda: lib.ao_codebook_assign(None, None, None, 0, 8, 256, None), lambda: lib.ao_codebook_pack_u4(None, None, 0, None),
                 lambda: lib.ao_codebook_dequantize(None, None, None, None, 0, 64, 4, 256, 32, None),
                 lambda: lib.ao_codebook_linear(None, one, one, one, None, 0, 16, 64, 4, 256, 64, None)):
        assert call() == _lib.AO_OK


def test_route_at_below_and_above_the_seam():
    assert _lib.lib().ao_codebook_linear_set_form(0) == _lib.AO_OK
    for m in (1, SEAM):
        r = ops.codebook_linear_route(m, 4096, 4096, 8, 256, 4096)
        assert r["kernel"] == "codebook_stream_kernel" and r["grid"] == (256, 1) and r["m_tiles"] == (1 if m == 1 else 4)
    assert ops.codebook_linear_route(SEAM + 1, 4096, 4096, 8, 256, 4096)["kernel"] == "not fused"
    assert ops.codebook_linear_kernel_name(SEAM + 1, 4096, 4096, 8, 256, 4096) == "not fused"
    for d in (1, 2):  # the narrow blocks hand over at 48 rows
        assert ops.codebook_linear_kernel_name(48, 4096, 4096, d, 256, 4096) == "codebook_stream_kernel"
        assert ops.codebook_linear_kernel_name(49, 4096, 4096, d, 256, 4096) == "not fused"
    assert ops.codebook_linear_kernel_name(SEAM, 4096, 4096, 4, 16, 4096) == "codebook_stream_kernel"
    assert ops.codebook_linear_fits(1, 40, 416, 1, 16, 32) is None
    assert "multiples of 32" in ops.codebook_linear_fits(1, 40, 96, 4, 256, 48)  # sb off the 32 grid: dequantize, then multiply
    assert ops.codebook_linear_kernel_name(1, 40, 96, 4, 256, 48) == "not fused"
    ops.codebook_linear_set_form(1)
    try:
        assert ops.codebook_linear_kernel_name(SEAM + 1, 40, 416, 1, 16, 32) == "codebook_stream_kernel"
        assert ops.codebook_linear_kernel_name(1, 40, 96, 4, 256, 48) == "not fused"  # forcing does not widen what the kernel takes
    finally:
        ops.codebook_linear_set_form(0)
