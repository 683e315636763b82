"""W4A8 without a GPU: the ABI, the named refusals, the route, the restatement against the recorded bytes, the Gaussian bound, the handler."""
import os

import numpy as np
import pytest
import torch

import da8w4_ref as R
from ao_amd import _lib, ops
from ao_amd.prototype import Int4OpaqueTensor, Int8DynamicActivationInt4WeightConfig
from ao_amd.quantization import quantize_

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "da8w4.npz"))


def test_abi_is_declared_and_refuses_shapes_then_null_pointers():
    lib, declared = _lib.lib(), _lib.declared_symbols()
    for name in ("quantize_weight", "dequantize", "quantize_act", "linear_fits", "linear_route", "linear_kernel_name", "linear_set_form", "linear"):
        assert hasattr(lib, "ao_da8w4_" + name) and "ao_da8w4_" + name in declared and "ao_da8w4_" + name in _lib._SIGNATURES
        assert "da8w4_" + name in ops.__all__
    assert lib.ao_da8w4_linear(None, None, None, None, None, None, None, 4, 32, 96, 64, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert "K=96 must be a positive multiple of group_size=64" in _lib.last_error()
    assert lib.ao_da8w4_linear(None, None, None, None, None, None, None, 4, 32, 128, 64, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_da8w4_quantize_weight(None, None, None, None, None, 32, 64, 32, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_da8w4_quantize_act(None, None, None, None, None, 4, 64, 32, 0, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_da8w4_linear_set_form(3) == _lib.AO_ERR_INVALID_ARGUMENT and "form must be 0" in _lib.last_error()


def test_fits_names_each_refusal():
    for shape, word in (((4, 32, 256, 16), "group_size=16 must be 32, 64 or 128"), ((4, 32, 256, 256), "group_size=256 must be 32, 64 or 128"),
                        ((4, 32, 160, 64), "K=160 must be a positive multiple of group_size=64"), ((4, 48, 256, 32), "N=48 must be a positive multiple of 32"),
                        ((4, 32, 1 << 25, 32), "too large"), ((1 << 22, 32, 1024, 32), "M=4194304 too large")):
        assert word in ops.da8w4_linear_fits(*shape)
        assert ops.da8w4_linear_route(*shape)["kernel"] == "invalid" and ops.da8w4_linear_kernel_name(*shape) == "invalid"


def test_route_seam_and_grid():
    assert ops.da8w4_linear_fits(17, 96, 160, 32) is None
    r = ops.da8w4_linear_route(16, 4096, 4096, 128)
    assert (r["kernel"], r["waves"], r["tile_m"], r["tile_n"], r["grid"]) == ("da8w4_stream_kernel", 8, 16, 16, (256, 1))
    assert ops.da8w4_linear_route(64, 4096, 4096, 128)["grid"] == (256, 4)  # the seam: one m-tile a workgroup, more rows add grid rows
    r = ops.da8w4_linear_route(65, 4096, 4096, 128)
    assert (r["kernel"], r["waves"], r["tile_m"], r["tile_n"], r["grid"]) == ("da8w4_tile_kernel", 4, 128, 64, (64, 1))
    assert ops.da8w4_linear_route(129, 96, 160, 32)["grid"] == (2, 2)
    assert ops.da8w4_linear_route(1, 32, 160, 32)["waves"] == 2  # no wave without a 128-k step
    try:
        ops.da8w4_linear_set_form(1)
        r = ops.da8w4_linear_route(65, 96, 512, 64)
        assert r["kernel"] == "da8w4_stream_kernel" and r["grid"] == (6, 5)
        ops.da8w4_linear_set_form(2)
        assert ops.da8w4_linear_kernel_name(1, 96, 512, 64) == "da8w4_tile_kernel"
    finally:
        ops.da8w4_linear_set_form(0)


def test_restatement_reproduces_every_recorded_byte():
    for g in R.GROUPS:
        for k in (g, 3 * g):
            key = f"w_g{g}_k{k}"
            q, s, zp = R.weight_cast(GOLDEN["w"][:, :k], g)
            assert np.array_equal(q, GOLDEN[key + "_q"]) and np.array_equal(s, GOLDEN[key + "_s"]) and np.array_equal(zp, GOLDEN[key + "_zp"])
            assert q.max() <= 15 and zp.min() >= 0 and zp.max() <= 15
    assert {int(z) for z in GOLDEN["w_g32_k32_zp"][4:6, 0]} == {0, 15}  # the positive-only and the negative-only row
    for k in (32, 384):
        for mode in ("asym", "sym"):
            key = f"x_{mode}_k{k}"
            q, s, zp = R.act_cast(GOLDEN["x"][:, :k], mode == "sym")
            assert np.array_equal(q, GOLDEN[key + "_q"]) and np.array_equal(s, GOLDEN[key + "_s"]) and np.array_equal(zp, GOLDEN[key + "_zp"])


@pytest.mark.parametrize("g", R.GROUPS)
def test_fp32_chain_stays_inside_the_gaussian_bound(g):
    """the bound of test_da8w4_gpu's Gaussian case on an fp32 chain with MORE roundings than the kernels' (product and add rounded apart, where
    they use one fma a group).  The bound's 2^-8 |ref| term is exactly bf16's worst half-ulp, with no slack: the GPU run sits at 0.97 - 0.995 of
    the bound because of that one rounding, not of the summation order, whose share is the (G + 4) 2^-23 mag term."""
    rng = np.random.default_rng(g)
    k, m, n = 384 + g, 17, 96
    x_bits, w_bits, bias = (R.bf16.to_bits(R.bf16.bf16_round((rng.standard_normal(sh) * sc).astype(np.float32)))
                            for sh, sc in (((m, k), 3), ((n, k), 0.05), ((n,), 1)))
    qa, sa, za = R.act_cast(x_bits, False)
    qw, sw, zw = R.weight_cast(w_bits, g)
    ref, mag = R.linear64(qa, sa, za, qw, sw, zw, bias)
    acc = np.zeros((m, n), np.float32)
    for ig, s in zip(R.group_sums(qa, za, qw, zw), sw.T):
        acc = acc + ig.astype(np.float32) * s[None, :]
    y = R.bf16.bf16_round(acc * sa[:, None] + R.bf16.from_bits(bias)[None, :]).astype(np.float64)
    assert np.all(np.abs(y - ref) <= R.bound(ref, mag, k // g))


def test_handler_skips_what_the_format_does_not_take_and_from_hp_is_refused():
    for lin, cfg in ((torch.nn.Linear(96, 32, dtype=torch.bfloat16), Int8DynamicActivationInt4WeightConfig(group_size=64)),
                     (torch.nn.Linear(64, 32, dtype=torch.bfloat16), Int8DynamicActivationInt4WeightConfig(group_size=16)),
                     (torch.nn.Linear(64, 48, dtype=torch.bfloat16), Int8DynamicActivationInt4WeightConfig())):
        quantize_(lin, cfg)
        assert type(lin.weight.data) is torch.Tensor and not isinstance(lin.weight, Int4OpaqueTensor)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        quantize_(torch.nn.Linear(64, 32, dtype=torch.bfloat16), Int8DynamicActivationInt4WeightConfig())
    with pytest.raises(NotImplementedError, match="Int4WeightOnlyConfig"):
        Int4OpaqueTensor.from_hp(torch.zeros(32, 64, dtype=torch.bfloat16), [1, 32])
