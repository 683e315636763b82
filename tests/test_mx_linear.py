"""MX dense linears without a GPU: the test oracle against the reference's fixture, the C ABI's new entries (exports, argument checks,
the route), the config and the fake kernels (tests/mx_linear_ref.py, tests/golden/mx_linear.npz)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_linear_ref as R  # noqa: E402

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mx_linear.npz"))
NEW = ["ao_mxfp4_quantize_rowwise", "ao_mx_linear", "ao_mx_dynamic_linear_fits", "ao_mx_dynamic_linear", "ao_mx_linear_route",
       "ao_mx_linear_kernel_name", "ao_mx_linear_set_form"]


def _lib():
    from ao_amd import _lib

    return _lib.lib()


@pytest.mark.parametrize("name", ["seeded", "edge"])
@pytest.mark.parametrize("tag,fmt", [("fp4", R.FMT_E2M1), ("fp8", R.FMT_E4M3)])
@pytest.mark.parametrize("mode_name,mode", [("floor", R.FLOOR), ("rceil", R.RCEIL)])
def test_oracle_cast_reproduces_fixture(name, tag, fmt, mode_name, mode):
    q, s = R.quantize(GOLDEN[f"{name}_x"], fmt, mode)
    np.testing.assert_array_equal(q, GOLDEN[f"{name}_{tag}_{mode_name}_q"])
    np.testing.assert_array_equal(s, GOLDEN[f"{name}_{tag}_{mode_name}_s"])


@pytest.mark.parametrize("tag,fmt", [("fp4", R.FMT_E2M1), ("fp8", R.FMT_E4M3)])
def test_oracle_dequantize_and_emulated_linear_reproduce_fixture(tag, fmt):
    nan = lambda b: (b & 0x7FFF) > 0x7F80  # noqa: E731
    for name, key in (("seeded", "dequant_"), ("edge", "dequant_edge_")):
        q, s = R.quantize(GOLDEN[f"{name}_x"], fmt, R.RCEIL)
        d, ref = R.dequantize_bf16(q, s, fmt), GOLDEN[key + tag]
        np.testing.assert_array_equal(nan(d), nan(ref))
        np.testing.assert_array_equal(np.where(nan(d), 0, d), np.where(nan(ref), 0, ref))
    aq, a_s = R.quantize(GOLDEN["lin_x"], fmt, R.RCEIL)
    wq, ws = R.quantize(GOLDEN["lin_w"], fmt, R.RCEIL)
    np.testing.assert_array_equal(R.emulated_linear_bf16(aq, a_s, wq, ws, fmt), GOLDEN[f"lin_{tag}_nobias"])
    np.testing.assert_array_equal(R.emulated_linear_bf16(aq, a_s, wq, ws, fmt, GOLDEN["lin_b"]), GOLDEN[f"lin_{tag}_bias"])
    # the reference's transform stores swizzled scales padded to 128 x 4 blocks; this backend keeps [48, 4] row-major
    np.testing.assert_array_equal(GOLDEN[f"lin_{tag}_w_scale_shape"], [32, 16])


def test_oracle_e2m1_rounding_points():
    x = np.array([0.25, 0.75, 5.0, 7.0, -0.0, 1.25, 1.75, 2.5, 3.5, 6.0, 100.0, -0.25, 0.2], dtype=np.float32)
    codes = R.f32_to_e2m1(x.view(np.uint32))
    np.testing.assert_array_equal(R.E2M1_VALUES[codes], [0.0, 1.0, 4.0, 6.0, -0.0, 1.0, 2.0, 2.0, 4.0, 6.0, 6.0, -0.0, 0.0])
    assert codes[4] == 8 and codes[11] == 8  # the sign of -0 is kept


def test_new_symbols_exported_and_abi_version_kept():
    from ao_amd import _lib

    lib = _lib.lib()
    assert lib.ao_abi_version() == 2
    declared = set(_lib.declared_symbols())
    for name in NEW:
        assert name in declared and name in _lib._SIGNATURES
        assert hasattr(lib, name)


def test_bad_arguments_refused_without_launch():
    from ao_amd import _lib

    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    for fmt, M, N, K in ((4, 4, 16, 48), (4, 4, 0, 64), (4, -1, 16, 64), (1, 4, 16, 64), (0, 4, 16, 0)):
        assert lib.ao_mx_linear(fmt, p, p, p, p, None, p, M, N, K, None) == _lib.AO_ERR_INVALID_ARGUMENT
        assert lib.ao_mx_dynamic_linear(fmt, p, p, p, None, p, M, N, K, 1, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_mx_linear(4, None, p, p, p, None, p, 4, 16, 64, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_mx_linear(4, p, p, None, p, None, p, 4, 16, 64, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_mx_linear(0, p, p, p, p, None, None, 4, 16, 64, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_mx_dynamic_linear(4, None, p, p, None, p, 4, 16, 64, 1, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_mx_dynamic_linear(4, p, p, p, None, p, 4, 16, 64, 7, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_mx_dynamic_linear(4, p, p, p, None, p, 500, 16, 64, 1, None) == _lib.AO_ERR_INVALID_ARGUMENT  # the tiled form
    assert lib.ao_mxfp4_quantize_rowwise(p, p, p, 4, 48, 1, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_mxfp4_quantize_rowwise(p, p, p, 4, 64, 2, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_mxfp4_quantize_rowwise(None, p, p, 4, 64, 1, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_mx_linear_route(4, 1, 16, 64, None, 7) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_mx_linear_set_form(3) == _lib.AO_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("fmt", [R.FMT_E2M1, R.FMT_E4M3])
def test_route_grid(fmt):
    from ao_amd import ops

    for M in (0, 1, 2, 15, 16, 17, 32, 33, 63, 64, 65, 128, 129, 2048, 16384):
        for N in (1, 17, 1024, 4096, 14336):
            for K in (32, 96, 4096, 14336):
                r = ops.mx_linear_route(fmt, M, N, K)
                name = ops.mx_linear_kernel_name(fmt, M, N, K)
                assert r["kernel"] == name
                seam = 32 if fmt == R.FMT_E2M1 else 64  # include/ao_mi355.h, DESIGN.md 4.10
                assert name == ("mx_linear_stream_kernel" if M <= seam else "mx_linear_tile_kernel"), (M, N, K)
                assert bool(_lib().ao_mx_dynamic_linear_fits(fmt, M, N, K)) == (M <= seam)
                if name == "mx_linear_stream_kernel":
                    assert r["tile_n"] == 16 and r["waves"] in (1, 2, 4, 8, 16) and r["grid"][0] == (N + 15) // 16
                    assert r["m_tiles"] * 16 * r["grid"][1] >= M and r["waves"] * r["m_tiles"] <= 32
                    assert r["waves"] <= max(1, (K + 127) // 128)
                else:
                    assert r["tile_m"] == r["tile_n"] == 128 and r["grid"] == ((N + 127) // 128, (M + 127) // 128)
    for bad in ((fmt, 1, 16, 48), (fmt, 1, 0, 64), (1, 1, 16, 64), (fmt, -1, 16, 64)):
        assert ops.mx_linear_kernel_name(*bad) == "invalid"


def test_forced_form_is_reported():
    from ao_amd import ops

    try:
        ops.mx_linear_set_form(2)
        assert ops.mx_linear_kernel_name(4, 1, 4096, 4096) == "mx_linear_tile_kernel"
        ops.mx_linear_set_form(1)
        assert ops.mx_linear_kernel_name(4, 4096, 4096, 4096) == "mx_linear_stream_kernel"
    finally:
        ops.mx_linear_set_form(0)
    assert ops.mx_linear_kernel_name(4, 1, 4096, 4096) == "mx_linear_stream_kernel"


def test_config_round_trip_and_asserts():
    from ao_amd.prototype import mx
    from ao_amd.quantization import KernelPreference, config_from_dict, config_to_dict

    for elem in (torch.float8_e4m3fn, torch.float4_e2m1fn_x2):
        c = mx.MXDynamicActivationMXWeightConfig(activation_dtype=elem, weight_dtype=elem)
        assert c.block_size == 32 and c.kernel_preference == KernelPreference.AUTO and c.scaling_mode == mx.ScaleCalculationMode.RCEIL
        assert config_from_dict(config_to_dict(c)) == c
    default = mx.MXDynamicActivationMXWeightConfig()
    assert default.activation_dtype == default.weight_dtype == torch.float8_e4m3fn
    with pytest.raises(AssertionError):
        mx.MXDynamicActivationMXWeightConfig(activation_dtype=torch.float8_e4m3fn, weight_dtype=torch.float4_e2m1fn_x2)
    with pytest.raises(NotImplementedError):
        mx.MXDynamicActivationMXWeightConfig(activation_dtype=torch.float8_e5m2, weight_dtype=torch.float8_e5m2)
    k = mx.QuantizeTensorToMXKwargs()
    assert (k.elem_dtype, k.block_size, k.scaling_mode, k.kernel_preference, k.is_swizzled_scales) == (
        torch.float8_e4m3fn, 32, mx.ScaleCalculationMode.FLOOR, KernelPreference.EMULATED, False)
    from ao_amd.quantization.quant_api import _QUANTIZE_CONFIG_HANDLER

    assert mx.MXDynamicActivationMXWeightConfig in _QUANTIZE_CONFIG_HANDLER


def test_to_mx_still_refuses_e5m2():
    from ao_amd.prototype import mx

    with pytest.raises(NotImplementedError):
        mx.to_mx(torch.zeros(2, 32, dtype=torch.bfloat16), torch.float8_e5m2)


def test_fake_kernels_on_meta():
    import ao_amd.torch_ops  # noqa: F401

    x = torch.empty(5, 256, dtype=torch.bfloat16, device="meta")
    q, s = torch.ops.ao_mi355.mxfp4_quantize(x, "rceil")
    assert q.shape == (5, 128) and q.dtype == torch.uint8 and s.shape == (5, 8) and s.dtype == torch.float8_e8m0fnu
    w4 = torch.empty(96, 128, dtype=torch.uint8, device="meta")
    ws = torch.empty(96, 8, dtype=torch.float8_e8m0fnu, device="meta")
    y = torch.ops.ao_mi355.mx_linear(x, w4, ws, None, 4, "rceil")
    assert y.shape == (5, 96) and y.dtype == torch.bfloat16
    y = torch.ops.ao_mi355.mx_mm(q, s, w4, ws, None, 4)
    assert y.shape == (5, 96) and y.dtype == torch.bfloat16


def test_mxtensor_reports_hp_shape_on_meta():
    from ao_amd.prototype.mx import MXTensor
    from ao_amd.quantization import KernelPreference

    q = torch.empty(48, 64, dtype=torch.uint8, device="meta")
    s = torch.empty(48, 4, dtype=torch.float8_e8m0fnu, device="meta")
    t = MXTensor(q, s, torch.float4_e2m1fn_x2, 32, torch.bfloat16, KernelPreference.AUTO, None, False)
    assert t.shape == (48, 128) and t.dtype == torch.bfloat16
    tt = t.t()
    assert tt.shape == (128, 48) and tt.qdata.shape == (64, 48)
    assert tt.t().shape == (48, 128)
