"""CPU: AWQ's restatement against the fixture recorded from the reference's observer, the config, the refusals, the entry's argument rules,
the observer's sums.  No kernel runs here."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import awq_ref as R
from ao_amd import _lib, ops, prototype
from ao_amd.prototype import MXFP8TrainingOpConfig, NVFP4WeightOnlyConfig
from ao_amd.prototype.awq import AWQConfig, AWQObservedLinear, AWQObserver
from ao_amd.prototype.nvfp4_tensor import QuantizationStep
from ao_amd.quantization import quantize_
from ao_amd.quantization.config import (
    Float8DynamicActivationInt4WeightConfig,
    Float8WeightOnlyConfig,
    Int4WeightOnlyConfig,
    Int8WeightOnlyConfig,
    config_from_dict,
    config_to_dict,
)
from oracle import bf16

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "awq.npz"))
META = json.loads(str(GOLDEN["meta"]))
BASE = Int4WeightOnlyConfig(group_size=32, int4_packing_format="plain")


def test_restatement_equals_the_fixture_byte_for_byte():
    """the scaled weights the reference handed to its quantizer and the dequantized weights it got back, all R of them"""
    got = R.chain(GOLDEN["W"], GOLDEN["S"], META["g"])
    assert got["ws"].shape == (META["R"], META["N"], META["K"])
    assert np.array_equal(bf16.to_bits(got["ws"]), GOLDEN["ws_bits"])
    assert np.array_equal(bf16.to_bits(got["dq"]), GOLDEN["dq_bits"])
    assert np.all(GOLDEN["S"][0] == 1) and np.array_equal(GOLDEN["S"][int(GOLDEN["best_index"])], GOLDEN["best_scales"])
    D = got["D"]
    assert D.dtype == np.float32 and np.array_equal(D, (GOLDEN["W"][None] - (got["dq"] / GOLDEN["S"][:, None, :]).astype(np.float32)))
    assert np.all(D[:, 2, 32:64] == 0)  # the all-zero group: s = 1e-6 / 15, every code is the zero point's, dq = 0


def test_x_mean_of_the_running_sum_is_the_fixtures():
    """fp32 sum of |x| over the batches, divided once, rounded once: within one bf16 ulp of the reference's mean of the bf16 inputs"""
    X = torch.from_numpy(GOLDEN["X"]).to(torch.bfloat16)
    obs = AWQObserver(torch.from_numpy(GOLDEN["W"]).to(torch.bfloat16), None, BASE)
    r0 = 0
    for b in META["batches"]:
        obs(X[r0:r0 + b], None)
        r0 += b
    assert obs.rows == sum(META["batches"]) and isinstance(obs.rows, int)
    got, want = bf16.to_bits(obs.get_act_scale().float().numpy()).astype(np.int64), bf16.to_bits(GOLDEN["x_mean"]).astype(np.int64)
    assert np.abs(got - want).max() <= 1  # positive bf16 values: adjacent bit patterns are adjacent values
    G = GOLDEN["X"].astype(np.float64).T @ GOLDEN["X"].astype(np.float64)
    np.testing.assert_allclose(obs.gram.numpy(), G, rtol=0, atol=1e-5 * np.abs(G).max())


def test_gram_form_of_the_loss_is_the_reference_formula():
    """tr(D G D^T) / (rows N) == mean((X D^T)^2) in float64, to 1e-12 relative, for every ratio of the fixture"""
    a = R.losses64(GOLDEN["W"], GOLDEN["S"], META["g"], GOLDEN["X"])
    b = R.gram_losses64(GOLDEN["W"], GOLDEN["S"], META["g"], GOLDEN["X"])
    assert a.shape == (META["R"],) and np.all(a > 0)
    assert np.abs(a - b).max() <= 1e-12 * a.max() and np.all(np.abs(a - b) <= 1e-12 * a)
    assert int(np.argmin(a)) == int(GOLDEN["best_index"])  # on this fixture the reference's bf16 losses pick the float64 minimum


def test_step_is_lower_cased_and_validated():
    assert AWQConfig(BASE, step="PREPARE").step == "prepare" and AWQConfig(BASE, "Convert").step == QuantizationStep.CONVERT
    assert AWQConfig(BASE, QuantizationStep.PREPARE_FOR_LOADING).step == "prepare_for_loading"
    assert AWQConfig(BASE, "prepare").scale_search_space_size == 20
    assert [s.value for s in QuantizationStep] == ["prepare", "convert", "prepare_for_loading"]
    with pytest.raises(ValueError, match="calibrate is not one of"):
        AWQConfig(BASE, step="calibrate")


def test_config_round_trip():
    c = AWQConfig(Int4WeightOnlyConfig(group_size=64), step="convert", scale_search_space_size=10)
    d = json.loads(json.dumps(config_to_dict(c)))
    assert d["_type"] == "AWQConfig" and d["_data"]["base_config"]["_type"] == "Int4WeightOnlyConfig" and d["_data"]["step"] == "convert"
    back = config_from_dict(d)
    assert back == c and back.base_config.group_size == 64 and isinstance(back.base_config, Int4WeightOnlyConfig)


def test_exports():
    assert "awq_scaled_error" in ops.__all__
    for name in ("AWQConfig", "AWQObserver", "AWQObservedLinear"):
        assert name in prototype.__all__ and getattr(prototype, name) is getattr(prototype.awq, name)
    assert "ao_awq_scaled_error" in _lib.declared_symbols()


REFUSED = [
    (Int4WeightOnlyConfig(group_size=32, int4_packing_format="tile_packed_to_4d"), "PLAIN"),
    (Int4WeightOnlyConfig(group_size=32, int4_packing_format="preshuffled"), "'preshuffled'"),
    (Int4WeightOnlyConfig(group_size=32, int4_packing_format="plain_int32"), "'plain_int32'"),
    (Int4WeightOnlyConfig(group_size=32, int4_choose_qparams_algorithm="hqq"), "HQQ"),
    (Int4WeightOnlyConfig(group_size=16), "group_size 16"),
    (Float8DynamicActivationInt4WeightConfig(int4_packing_format="plain"), "fp8-activation"),
    (Int8WeightOnlyConfig(), "unsupported base_config Int8WeightOnlyConfig"),
    (Float8WeightOnlyConfig(), "unsupported base_config Float8WeightOnlyConfig"),
    (NVFP4WeightOnlyConfig(), "unsupported base_config NVFP4WeightOnlyConfig"),
    (MXFP8TrainingOpConfig(), "unsupported base_config MXFP8TrainingOpConfig"),
]


@pytest.mark.parametrize("base,frag", REFUSED, ids=[f for _, f in REFUSED])
def test_unsupported_bases_are_refused_by_name_at_prepare(base, frag):
    m = nn.Sequential(nn.Linear(64, 16, bias=False)).to(torch.bfloat16)
    for step in ("prepare", "prepare_for_loading"):
        with pytest.raises(NotImplementedError, match=frag) as e:
            quantize_(m, AWQConfig(base, step=step))
        assert "supports Int4WeightOnlyConfig(int4_packing_format='plain')" in str(e.value)
    assert type(m[0]) is nn.Linear


def test_unsupported_weights_are_refused_at_prepare():
    with pytest.raises(NotImplementedError, match="bfloat16 weights, got torch.float32"):
        quantize_(nn.Sequential(nn.Linear(64, 16)), AWQConfig(BASE, "prepare"))
    m = nn.Sequential(nn.Linear(48, 16)).to(torch.bfloat16)
    with pytest.raises(NotImplementedError, match="K=48 is not a multiple of group_size=32"):  # refused, not silently skipped
        quantize_(m, AWQConfig(BASE, "prepare"))
    lin = nn.Linear(64, 16).to(torch.bfloat16)
    lin.weight = nn.Parameter(torch.zeros(2, 16, 64, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="3-D expert weights"):
        quantize_(nn.Sequential(lin), AWQConfig(BASE, "prepare"))
    with pytest.raises(NotImplementedError, match="2-D linear weights"):
        AWQObserver(torch.zeros(2, 16, 64, dtype=torch.bfloat16), None, BASE)


def test_entry_checks_its_arguments_before_the_gpu():
    lib = _lib.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    f = lib.ao_awq_scaled_error
    assert f(one, one, one, 4, 96, 2, 64, None) == _lib.AO_ERR_INVALID_ARGUMENT and "multiple of group_size" in _lib.last_error()
    assert f(one, one, one, 4, 128, 2, 16, None) == _lib.AO_ERR_INVALID_ARGUMENT and "one of 32, 64, 128, 256" in _lib.last_error()
    assert f(one, one, one, 4, 128, 2, 48, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert f(one, one, one, -1, 128, 2, 32, None) == _lib.AO_ERR_INVALID_ARGUMENT and "bad shape" in _lib.last_error()
    assert f(one, one, one, 4, 0, 2, 32, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert f(one, one, one, 4, 128, -1, 32, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert f(one, one, one, 1 << 40, 1 << 20, 20, 32, None) == _lib.AO_ERR_INVALID_ARGUMENT and "too large" in _lib.last_error()
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert f(*args, 4, 128, 2, 32, None) == _lib.AO_ERR_NULL_POINTER
    assert f(ctypes.c_void_p(8), one, one, 4, 128, 2, 32, None) == _lib.AO_ERR_INVALID_ARGUMENT and "16-byte aligned" in _lib.last_error()
    assert f(None, None, None, 0, 128, 2, 32, None) == _lib.AO_OK  # nothing to do: nothing is touched
    assert f(None, None, None, 4, 128, 0, 32, None) == _lib.AO_OK
    assert f(None, None, None, 0, 96, 2, 64, None) == _lib.AO_ERR_INVALID_ARGUMENT  # the shape rules hold for an empty call too


def test_op_checks_its_arguments():
    W, S = torch.zeros(4, 128, dtype=torch.bfloat16), torch.ones(2, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.awq_scaled_error(W, S, 32)


def test_observer_sums_and_the_observed_linear():
    """forward returns the plain linear; abs_sum and gram are the unnormalised sums over 2-D and 3-D batches; the count is a host int"""
    gen = torch.Generator().manual_seed(5)
    m = nn.Sequential(nn.Linear(64, 8, bias=True)).to(torch.bfloat16)
    w, b = m[0].weight, m[0].bias
    quantize_(m, AWQConfig(BASE, "prepare", scale_search_space_size=7))
    obs = m[0].act_obs
    assert isinstance(m[0], AWQObservedLinear) and isinstance(obs, AWQObserver) and m[0].weight is w and m[0].bias is b
    assert obs.scale_options == 7 and obs.gram.shape == (64, 64) and obs.gram.dtype == torch.float32 and obs.rows == 0
    assert "act_obs.gram" not in m[0].state_dict() and "act_obs.abs_sum" not in m[0].state_dict()
    xs = [torch.randn(5, 64, generator=gen).bfloat16(), torch.randn(3, 4, 64, generator=gen).bfloat16(), torch.randn(7, 64, generator=gen).bfloat16()]
    for x in xs:
        assert torch.equal(m(x), torch.nn.functional.linear(x, w, b))
    X = torch.cat([x.reshape(-1, 64) for x in xs]).double().numpy()
    assert obs.rows == 24 and type(obs.rows) is int
    np.testing.assert_allclose(obs.abs_sum.numpy(), np.abs(X).sum(0), rtol=1e-6)
    np.testing.assert_allclose(obs.gram.numpy(), X.T @ X, rtol=0, atol=1e-6 * np.abs(X.T @ X).max())
    S = obs.scale_table(obs.get_act_scale())
    assert S.shape == (7, 64) and S.dtype == torch.bfloat16 and torch.all(S[0] == 1) and torch.all(S > 0)


def test_convert_without_calibration_raises_and_plain_linears_pass():
    m = nn.Sequential(nn.Linear(64, 8)).to(torch.bfloat16)
    plain = m[0]
    quantize_(m, AWQConfig(BASE, "convert"))
    assert m[0] is plain and type(m[0].weight) is nn.Parameter
    quantize_(m, AWQConfig(BASE, "prepare"))
    with pytest.raises(ValueError, match="calibrate observer first by running model on exemplar data"):
        quantize_(m, AWQConfig(BASE, "convert"))
    assert isinstance(m[0], AWQObservedLinear)
