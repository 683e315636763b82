"""NVFP4 linears, the parts that need no GPU: the restated arithmetic (tests/nvfp4_ref.py) against the reference's recorded bytes
(tests/golden/nvfp4.npz), the configs and their handlers' refusals, serialisation, the un-swizzle of a reference-layout scale tensor, the
C ABI's argument checks, the route query and the committed case list (tests/nvfp4_cases.py)."""
import ctypes
import dataclasses
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nvfp4_cases as nc
import nvfp4_ref as R
from ao_amd import _lib, ops
from ao_amd.prototype import (NVFP4DynamicActivationNVFP4WeightConfig, NVFP4Tensor, NVFP4WeightOnlyConfig, QuantizeTensorToNVFP4Kwargs,
                              per_tensor_amax_to_scale)
from ao_amd.prototype.nvfp4_tensor import QuantizationStep
from ao_amd.quantization import quant_api, quantize_

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "nvfp4.npz"))
NEW = ["ao_nvfp4_amax_scale", "ao_nvfp4_quantize", "ao_nvfp4_wo_linear", "ao_nvfp4_linear", "ao_nvfp4_linear_route",
       "ao_nvfp4_linear_kernel_name", "ao_nvfp4_linear_set_form"]
MATRICES = ["cast", "edge", "nonf"]
MODES = ["none", "given", "dyn"]


def bf(name):
    return torch.from_numpy(GOLDEN[name].view(np.int16).copy()).view(torch.bfloat16)


def u8(name):
    return torch.from_numpy(GOLDEN[name].copy())


def f32(name):
    return torch.tensor(float(GOLDEN[name]), dtype=torch.float32)


def per_tensor(name, mode):
    return {"none": None, "given": f32("given_p"), "dyn": torch.from_numpy(GOLDEN[f"{name}_dyn_p"].copy())}[mode]


# ---- the oracle equals the fixture byte for byte ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", MATRICES)
def test_ref_cast_reproduces_the_reference_bytes(name, mode):
    q, s = R.cast(bf(f"{name}_x"), per_tensor(name, mode))
    assert torch.equal(q, u8(f"{name}_{mode}_q")) and torch.equal(s, u8(f"{name}_{mode}_s"))


@pytest.mark.parametrize("name", MATRICES)
def test_ref_amax_scale_reproduces_the_reference_bits(name):
    got, want = R.amax_scale(bf(f"{name}_x")), torch.from_numpy(GOLDEN[f"{name}_dyn_p"].copy())
    assert got.view(torch.int32).item() == want.view(torch.int32).item()
    assert torch.equal(per_tensor_amax_to_scale(torch.tensor(5376.0)), torch.tensor(2.0))


def test_fixture_holds_the_edge_blocks_it_names():
    s = GOLDEN["edge_none_s"].reshape(-1).tolist()
    assert s[0] == 8 and s[1] == 8                      # all-zero and all -0.0: the scale's floor 2^-6
    assert GOLDEN["edge_none_q"][1].tolist() == [0x88] * 8  # -0.0 keeps its sign
    assert s[5:11] == [56, 56, 57, 57, 58, 58]          # below / at (to even) / above the ties 1.0625 and 1.1875
    assert s[13:18] == [126] * 5                        # saturated at 448
    assert GOLDEN["nonf_none_s"].reshape(-1).tolist()[:5] == [126, 126, 127, 127, 127]
    assert np.isnan(GOLDEN["nonf_dyn_p"]) and GOLDEN["nonf_dyn_s"].reshape(-1).tolist() == [127] * 6


@pytest.mark.parametrize("mode", ["none", "given"])
def test_ref_dequantize_reproduces_the_reference_bits(mode):
    p = per_tensor("cast", mode)
    d = R.dequantize(u8(f"cast_{mode}_q"), u8(f"cast_{mode}_s"), p)
    assert torch.equal(R.bits(d), R.bits(bf(f"deq_{mode}")))
    t = NVFP4Tensor(u8(f"cast_{mode}_q"), u8(f"cast_{mode}_s").view(torch.float8_e4m3fn), 16, torch.bfloat16, p)
    assert tuple(t.shape) == (12, 64) and t.dtype == torch.bfloat16
    assert torch.equal(R.bits(t.dequantize()), R.bits(bf(f"deq_{mode}")))
    assert torch.equal(R.bits(t.t().dequantize()), R.bits(bf(f"deq_{mode}").t().contiguous()))
    assert torch.equal(t.get_hp_scales(), R.scales32(u8(f"cast_{mode}_s"), p))
    if mode == "none":  # code x block scale is exact in bf16
        assert torch.equal(t.dequantize(torch.float32), t.dequantize(torch.float32).to(torch.bfloat16).float())


@pytest.mark.parametrize("tag", ["nop", "p"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_ref_weight_only_linear_reproduces_the_reference_bit_for_bit(tag, with_bias):
    p = f32("lin_p") if tag == "p" else None
    y = R.wo_linear(bf("lin_x"), u8("lin_q"), u8("lin_s"), p, bf("lin_bias") if with_bias else None)
    assert torch.equal(R.bits(y), R.bits(bf(f"lin_{tag}_y" if with_bias else f"lin_{tag}_y_nobias")))


def test_golden_linear_inputs_have_exact_sums():
    x = bf("lin_x").double()
    assert float(x.abs().max()) <= 8 and torch.equal(x, x.round())
    s = u8("lin_s").view(torch.float8_e4m3fn).double()
    assert set(s.reshape(-1).tolist()) <= {0.25, 0.5, 1.0, 2.0}
    assert x.shape[1] * 8 * 6 * 2 * 8 <= 2 ** 24  # terms are multiples of 2^-3 (2^-6 under p = 2^-3), |term| <= 96


# ---- the tensor, the configs and their handlers -----------------------------------------------------------------------------------------
def test_kwargs_and_config_defaults():
    k = QuantizeTensorToNVFP4Kwargs()
    assert (k.block_size, k.is_swizzled_scales, k.use_triton_kernel, k.use_dynamic_per_tensor_scale) == (16, False, False, False)
    assert [f.name for f in dataclasses.fields(k)] == ["block_size", "is_swizzled_scales", "use_triton_kernel", "use_dynamic_per_tensor_scale"]
    d = NVFP4DynamicActivationNVFP4WeightConfig()
    assert (d.use_triton_kernel, d.use_dynamic_per_tensor_scale, d.step) == (True, True, None)
    assert [f.name for f in dataclasses.fields(d)] == ["use_triton_kernel", "use_dynamic_per_tensor_scale", "step"]
    s = NVFP4DynamicActivationNVFP4WeightConfig(step="prepare")
    assert s.step is QuantizationStep.PREPARE and s.use_dynamic_per_tensor_scale is False
    w = NVFP4WeightOnlyConfig()
    assert w.use_dynamic_per_tensor_scale is True and [f.name for f in dataclasses.fields(w)] == ["use_dynamic_per_tensor_scale"]
    for cls in (NVFP4DynamicActivationNVFP4WeightConfig, NVFP4WeightOnlyConfig):
        assert cls in quant_api._QUANTIZE_CONFIG_HANDLER
    assert NVFP4Tensor.tensor_data_names == ["qdata", "scale"]
    assert NVFP4Tensor.optional_tensor_data_names == ["per_tensor_scale", "act_per_tensor_scale"]


@pytest.mark.parametrize("cfg", [NVFP4WeightOnlyConfig(), NVFP4DynamicActivationNVFP4WeightConfig()])
def test_handlers_refuse_with_the_reason(cfg):
    for shape in ((24, 64), (32, 40)):
        lin = torch.nn.Linear(shape[1], shape[0], dtype=torch.bfloat16)
        with pytest.raises(RuntimeError, match="NVFP4 only supports weight shape with last 2 dims divisible by 16"):
            quantize_(lin, cfg)
        assert type(lin.weight) is torch.nn.Parameter
    with pytest.raises(NotImplementedError, match="takes bfloat16 weights"):
        quantize_(torch.nn.Linear(64, 32, dtype=torch.float32), cfg)


@pytest.mark.parametrize("step", ["prepare", "convert"])
def test_observer_flow_is_refused(step):
    with pytest.raises(NotImplementedError, match="observer flow"):
        quantize_(torch.nn.Linear(64, 32, dtype=torch.bfloat16), NVFP4DynamicActivationNVFP4WeightConfig(step=step))


def _weight(act_quant_kwargs=None, p=True):
    return NVFP4Tensor(u8("w48_q"), u8("w48_scale_row_major").view(torch.float8_e4m3fn), 16, torch.bfloat16,
                       torch.from_numpy(GOLDEN["w48_p"].copy()) if p else None, None, False, False, act_quant_kwargs)


def test_tensor_refusals_name_the_restriction():
    t = _weight()
    for dt in (torch.float32, torch.float16):
        with pytest.raises(NotImplementedError, match="takes bfloat16 activations"):
            F.linear(torch.zeros(2, 128, dtype=dt), t)
    with pytest.raises(NotImplementedError, match="takes bfloat16 tensors"):
        NVFP4Tensor.to_nvfp4(torch.zeros(16, 32))
    with pytest.raises(NotImplementedError, match="3-D"):
        NVFP4Tensor.to_nvfp4(torch.zeros(2, 16, 32, dtype=torch.bfloat16))
    with pytest.raises(AssertionError, match="row-major scales"):
        NVFP4Tensor(u8("w48_q"), u8("w48_scale_swizzled").view(torch.float8_e4m3fn), 16, torch.bfloat16, None, None, True)
    with pytest.raises(NotImplementedError, match="per-expert"):
        NVFP4Tensor(u8("w48_q"), u8("w48_scale_row_major").view(torch.float8_e4m3fn), 16, torch.bfloat16, torch.ones(2, 1, 1))
    with pytest.raises(NotImplementedError, match="dim 0 only"):
        t[:, :64]


def test_views_and_row_slices():
    t = _weight(QuantizeTensorToNVFP4Kwargs(use_dynamic_per_tensor_scale=True))
    assert tuple(t.shape) == (48, 128) and tuple(t.t().shape) == (128, 48) and tuple(t.t().t().shape) == (48, 128)
    s = t[16:40]
    assert isinstance(s, NVFP4Tensor) and tuple(s.shape) == (24, 128) and tuple(s.scale.shape) == (24, 8)
    assert s.act_quant_kwargs == t.act_quant_kwargs and s.per_tensor_scale is t.per_tensor_scale
    assert torch.equal(R.bits(s.dequantize()), R.bits(bf("w48_deq")[16:40]))
    v = t.view(48, 128)
    assert tuple(v.shape) == (48, 128) and tuple(v.qdata.shape) == (48, 64)
    assert "NVFP4Tensor" in repr(t)


def test_from_reference_layout_unswizzles_the_scale():
    p = torch.from_numpy(GOLDEN["w48_p"].copy())
    t = NVFP4Tensor.from_reference_layout(u8("w48_q"), u8("w48_scale_swizzled").view(torch.float8_e4m3fn), per_tensor_scale=p)
    assert t.is_swizzled_scales is False and tuple(t.scale.shape) == (48, 8) and t.scale.dtype == torch.float8_e4m3fn
    assert torch.equal(t.scale.view(torch.uint8), u8("w48_scale_row_major"))
    assert torch.equal(R.unswizzle(u8("w48_scale_swizzled"), 48, 8), u8("w48_scale_row_major"))
    assert torch.equal(R.bits(t.dequantize()), R.bits(bf("w48_deq")))
    # the reference's own cast of that weight, restated
    q, s = R.cast(bf("w48_w"), p)
    assert torch.equal(q, u8("w48_q")) and torch.equal(s, u8("w48_scale_row_major"))
    assert p.view(torch.int32).item() == R.amax_scale(bf("w48_w")).view(torch.int32).item()
    with pytest.raises(AssertionError, match="swizzled scale"):
        NVFP4Tensor.from_reference_layout(u8("w48_q"), u8("w48_scale_row_major"))


def test_safe_globals_round_trip():
    k = QuantizeTensorToNVFP4Kwargs(use_dynamic_per_tensor_scale=False)
    t = NVFP4Tensor(u8("w48_q"), u8("w48_scale_row_major").view(torch.float8_e4m3fn), 16, torch.bfloat16,
                    torch.from_numpy(GOLDEN["w48_p"].copy()), torch.tensor(0.5), False, True, k)
    buf = io.BytesIO()
    torch.save({"weight": t}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=True)["weight"]
    assert isinstance(back, NVFP4Tensor) and back.act_quant_kwargs == k and back.use_triton_kernel is True and back.block_size == 16
    assert torch.equal(back.qdata, t.qdata) and torch.equal(back.scale.view(torch.uint8), t.scale.view(torch.uint8))
    assert torch.equal(back.per_tensor_scale, t.per_tensor_scale) and torch.equal(back.act_per_tensor_scale, t.act_per_tensor_scale)
    assert back.orig_dtype == torch.bfloat16 and tuple(back.shape) == (48, 128)


# ---- the C ABI and the route --------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_new_symbols():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW:
        assert hasattr(lib, name) and name in declared and name in _lib._SIGNATURES
    for name in ("nvfp4_amax_scale", "nvfp4_quantize", "nvfp4_wo_linear", "nvfp4_mm", "nvfp4_linear_route", "nvfp4_linear_kernel_name",
                 "nvfp4_set_form"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    for name in ("nvfp4_amax_scale", "nvfp4_quantize", "nvfp4_wo_linear", "nvfp4_mm", "nvfp4_linear"):
        assert hasattr(torch.ops.ao_mi355, name)


def test_argument_checks_without_a_gpu():
    lib = _lib.lib()
    one = ctypes.c_void_p(4096)  # never dereferenced: validation fails first
    assert lib.ao_nvfp4_wo_linear(one, one, one, None, None, one, 4, 32, 24, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert "multiple of 16" in _lib.last_error()
    assert lib.ao_nvfp4_linear(one, one, None, one, one, None, None, one, 4, 0, 32, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_nvfp4_wo_linear(one, None, one, None, None, one, 4, 32, 32, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_nvfp4_linear(None, one, None, one, one, None, None, one, 4, 32, 32, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_nvfp4_wo_linear(None, one, one, None, None, None, 0, 32, 32, None) == _lib.AO_OK  # M = 0: nothing launched
    assert lib.ao_nvfp4_wo_linear(one, ctypes.c_void_p(4104), one, None, None, one, 4, 32, 32, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert "aligned" in _lib.last_error()
    assert lib.ao_nvfp4_quantize(one, None, one, one, 4, 24, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_nvfp4_quantize(None, None, None, None, 0, 32, None) == _lib.AO_OK
    assert lib.ao_nvfp4_amax_scale(one, None, 4, 32, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_nvfp4_linear_set_form(3) == _lib.AO_ERR_INVALID_ARGUMENT
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nvfp4_quantize(torch.zeros(4, 32, dtype=torch.bfloat16))


def test_route_seams_forms_and_invalid_shapes():
    for kind, k in (("wo", ops.NVFP4_KIND_WEIGHT_ONLY), ("dyn", ops.NVFP4_KIND_DYNAMIC)):
        assert ops.nvfp4_linear_route(k, 64, 4096, 4096)["kernel"] == "nvfp4_stream_kernel"
        assert ops.nvfp4_linear_route(k, 65, 4096, 4096)["kernel"] == "nvfp4_tile_kernel"
        assert ops.nvfp4_linear_kernel_name(k, 1, 4096, 4096) == "nvfp4_stream_kernel"
        r = ops.nvfp4_linear_route(k, 1, 4096, 4096)
        assert (r["waves"], r["m_tiles"], r["grid"]) == (8, 1, (256, 1))
        assert ops.nvfp4_linear_route(k, 100, 1000, 48) == {"kernel": "nvfp4_tile_kernel", "waves": 4, "m_tiles": 4, "tile_m": 64,
                                                            "tile_n": 64, "grid": (16, 2)}
        for bad in ((1, 16, 24), (1, 0, 32), (-1, 16, 32), (1, 16, 0), (1 << 20, 16, 1 << 12)):
            assert ops.nvfp4_linear_route(k, *bad)["kernel"] == "invalid"
            assert ops.nvfp4_linear_kernel_name(k, *bad) == "invalid"
        assert nc.route(_lib.lib(), kind, 33, 17, 144)["kernel"] == "stream"
    assert ops.nvfp4_linear_route(2, 1, 16, 32)["kernel"] == "invalid"
    ops.nvfp4_set_form(2)
    try:
        assert ops.nvfp4_linear_route(0, 1, 4096, 4096)["kernel"] == "nvfp4_tile_kernel"
    finally:
        ops.nvfp4_set_form(0)
    assert ops.nvfp4_linear_route(0, 1, 4096, 4096)["kernel"] == "nvfp4_stream_kernel"


def test_committed_cases_are_the_derivation():
    lib = _lib.lib()
    assert nc.CASES == nc.derive_cases(lib), "python tests/nvfp4_cases.py prints the list to commit"
    sigs = {nc.signature(lib, c) for c in nc.CASES}
    assert set(nc.reachable(lib)) <= sigs
    assert {s[:2] for s in sigs} == {(k, f) for k in nc.KIND for f in ("stream", "tile")}
    assert max(c[1] for c in nc.CASES) <= 257 and max(c[2] for c in nc.CASES) <= 1040 and max(c[3] for c in nc.CASES) <= 4096
    for c in nc.CASES:
        assert c[3] % 16 == 0
