"""CPU: GPTQ's restatement against the fixture recorded from the reference's pieces, the config, the refusals, the observer.  No kernel runs here."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import gptq_ref as R
from ao_amd import _lib
from ao_amd.prototype import NVFP4DynamicActivationNVFP4WeightConfig
from ao_amd.prototype.gptq import GPTQConfig, GPTQObserverTensor, gptq_quantize, gptq_quantize_3d
from ao_amd.quantization import quantize_
from ao_amd.quantization.config import (
    Float8DynamicActivationInt4WeightConfig,
    Float8WeightOnlyConfig,
    Int4WeightOnlyConfig,
    Int8WeightOnlyConfig,
    config_from_dict,
    config_to_dict,
)
from ao_amd.quantization.granularity import PerTensor

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gptq.npz"))
CASES = json.loads(str(GOLDEN["cases"]))


def _aux(c):
    key = f"{c['name']}_aux"
    if key not in GOLDEN.files:
        return None
    a = GOLDEN[key]
    return a.reshape(()) if c["fmt"] == R.NVFP4 else a


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_block_step_equals_the_fixture_byte_for_byte(c):
    """From the recorded state before every block (and the recorded Hinv: no factorization is involved) the restatement gives the
    reference's W, Err, qparams and final codes."""
    n = c["name"]
    blocks = 0
    for b, k0 in enumerate(range(0, c["K"], c["B"])):
        bw = min(c["B"], c["K"] - k0)
        step = R.block_step(GOLDEN[f"{n}_b{b}_Win"], c["bf16"], GOLDEN[f"{n}_Hinv"], k0, bw, c["fmt"], c["g"], _aux(c))
        assert _same(step["W"], GOLDEN[f"{n}_b{b}_Wstep"])
        assert _same(step["err"], GOLDEN[f"{n}_b{b}_err"])
        assert _same(step["qdata"], GOLDEN[f"{n}_b{b}_qdata"])
        for key in ("scale", "zero"):
            if f"{n}_b{b}_{key}" in GOLDEN.files:
                assert _same(step[key], GOLDEN[f"{n}_b{b}_{key}"])
        blocks += 1
    assert blocks == 2 and np.any(GOLDEN[f"{n}_b1_err"] != 0)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_scales_taken_before_the_loop(c):
    n = c["name"]
    if c["fmt"] == R.NVFP4:
        assert R.nvfp4_per_tensor_scale(GOLDEN[f"{n}_W0"]) == GOLDEN[f"{n}_aux"].reshape(())
    elif c["fmt"] == R.INT8:
        assert _same(R.int8_row_scale(GOLDEN[f"{n}_W0"], c["bf16"]), GOLDEN[f"{n}_aux"])


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_factorization_and_lazy_update_within_fp32_rounding(c):
    """The two steps a BLAS / LAPACK computes (their summation order is the library's, not the contract's): the restatement's own
    factorization lands on the recorded Hinv within fp32 rounding of a 64 x 64 problem, and the recorded lazy update is
    W - Err @ Hinv[k0:end, end:] within the fp32 summation bound of its 32-term sums plus the rounding into W's dtype."""
    n = c["name"]
    Hinv, W = R.factorize(GOLDEN[f"{n}_H"], GOLDEN[f"{n}_W0"], 0.01)
    want = GOLDEN[f"{n}_Hinv"]
    assert np.abs(Hinv - want).max() <= 1e-3 * np.abs(want).max()
    assert _same(W, GOLDEN[f"{n}_b0_Win"])  # the dead column went to zero
    assert np.all(W[:, 5] == 0) and np.any(GOLDEN[f"{n}_W0"][:, 5] != 0)
    k0, end = 0, c["B"]
    err = GOLDEN[f"{n}_b0_err"].astype(np.float64)
    h = want[k0:end, end:].astype(np.float64)
    before, after = GOLDEN[f"{n}_b0_Wstep"][:, end:].astype(np.float64), GOLDEN[f"{n}_b0_Wout"][:, end:].astype(np.float64)
    exact = before - err @ h
    bound = (c["B"] + 2) * 2.0 ** -23 * (np.abs(before) + np.abs(err) @ np.abs(h)) + (2.0 ** -8 * np.abs(exact) if c["bf16"] else 0)
    assert np.all(np.abs(after - exact) <= bound)
    assert _same(GOLDEN[f"{n}_b0_Wout"][:, :end], GOLDEN[f"{n}_b0_Wstep"][:, :end])  # the block's own columns are final


BASES = [Int4WeightOnlyConfig(group_size=32), Int8WeightOnlyConfig(), NVFP4DynamicActivationNVFP4WeightConfig()]


@pytest.mark.parametrize("base", BASES, ids=lambda b: type(b).__name__)
def test_config_round_trip(base):
    c = GPTQConfig(step="convert", base_config=base, percdamp=0.02, gptq_quantize_block_size=128)
    d = json.loads(json.dumps(config_to_dict(c)))
    assert d["_type"] == "GPTQConfig" and d["_data"]["base_config"]["_type"] == type(base).__name__
    assert config_from_dict(d) == c
    assert GPTQConfig(base_config=base).step == "observe" and GPTQConfig(base_config=base).gptq_quantize_block_size == 256


def test_config_requires_base_config():
    with pytest.raises(ValueError, match="base_config is required"):
        GPTQConfig(step="observe")


REFUSED = [
    (Int4WeightOnlyConfig(group_size=32, int4_packing_format="tile_packed_to_4d"), "PLAIN"),
    (Int4WeightOnlyConfig(group_size=32, int4_choose_qparams_algorithm="hqq"), "HQQ"),
    (Float8DynamicActivationInt4WeightConfig(int4_packing_format="plain"), "fp8-activation"),
    (Int8WeightOnlyConfig(granularity=PerTensor()), "per-row"),
    (NVFP4DynamicActivationNVFP4WeightConfig(use_dynamic_per_tensor_scale=False), "dynamic per-tensor scale"),
    (Float8WeightOnlyConfig(), "unsupported base_config"),
]


@pytest.mark.parametrize("base,frag", REFUSED, ids=[f for _, f in REFUSED])
def test_unsupported_targets_are_refused_by_name(base, frag):
    H, W = torch.eye(64), torch.zeros(16, 64, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match=frag):
        gptq_quantize(H, W, GPTQConfig("convert", base))
    m = nn.Sequential(nn.Linear(64, 16, bias=False)).to(torch.bfloat16)
    with pytest.raises(NotImplementedError, match=frag):  # refused before any calibration is spent
        quantize_(m, GPTQConfig("observe", base))


def test_3d_weights_and_other_dtypes_are_refused():
    cfg = GPTQConfig("convert", NVFP4DynamicActivationNVFP4WeightConfig())
    with pytest.raises(NotImplementedError, match="3-D expert weights"):
        gptq_quantize(torch.eye(64).repeat(2, 1, 1), torch.zeros(2, 16, 64, dtype=torch.bfloat16), cfg)
    with pytest.raises(NotImplementedError, match="gptq_quantize_3d"):
        gptq_quantize_3d(torch.eye(64).repeat(2, 1, 1), torch.zeros(2, 16, 64, dtype=torch.bfloat16), cfg)
    with pytest.raises(NotImplementedError, match="3-D expert weights"):
        GPTQObserverTensor.from_hp(torch.zeros(2, 16, 64, dtype=torch.bfloat16))
    obs = GPTQObserverTensor.from_hp(torch.zeros(16, 64))
    with pytest.raises(NotImplementedError, match="bmm / _grouped_mm"):
        torch.bmm(torch.zeros(1, 4, 16), obs)
    with pytest.raises(NotImplementedError, match="bmm / _grouped_mm"):
        obs.update_3d(torch.zeros(1, 4, 64))
    with pytest.raises(NotImplementedError, match="bfloat16 or float32"):
        gptq_quantize(torch.eye(64), torch.zeros(16, 64, dtype=torch.float16), cfg)


def test_block_size_rules():
    W = torch.zeros(16, 512, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="larger than 256"):
        gptq_quantize(torch.eye(512), W, GPTQConfig("convert", Int8WeightOnlyConfig(), gptq_quantize_block_size=512))
    with pytest.raises(ValueError, match="multiple of the group size"):
        gptq_quantize(torch.eye(512), W, GPTQConfig("convert", Int4WeightOnlyConfig(group_size=128), gptq_quantize_block_size=64))
    lib = _lib.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    assert lib.ao_gptq_block(one, 1, one, one, 0, 32, one, one, one, None, 4, 512, 0, 512, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert "1 .. 256 columns" in _lib.last_error()
    assert lib.ao_gptq_block(one, 1, one, one, 0, 128, one, one, one, None, 4, 512, 64, 128, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert "must start on a group" in _lib.last_error()
    assert lib.ao_gptq_block(one, 1, one, one, 0, 32, one, one, one, None, 4, 512, 448, 128, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_gptq_block(one, 1, None, one, 0, 32, one, one, one, None, 4, 512, 0, 128, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_gptq_block(one, 1, one, one, 2, 16, one, one, None, None, 4, 512, 0, 128, None) == _lib.AO_ERR_NULL_POINTER  # NVFP4: no p


def test_convert_needs_an_observer_with_batches():
    base = Int8WeightOnlyConfig()
    m = nn.Sequential(nn.Linear(64, 16, bias=False)).to(torch.bfloat16)
    with pytest.raises(ValueError, match="Did you run the 'observe' step first"):
        quantize_(m, GPTQConfig("convert", base))
    quantize_(m, GPTQConfig("observe", base))
    assert isinstance(m[0].weight, GPTQObserverTensor) and "GPTQObserverTensor" in repr(m)
    with pytest.raises(ValueError, match="total_batches is 0"):
        quantize_(m, GPTQConfig("convert", base))
    with pytest.raises(ValueError, match="Invalid step"):
        quantize_(m, GPTQConfig("calibrate", base))


def test_observer_running_mean_and_linear():
    """F.linear on the observer returns the plain linear and folds the input into H = (2 / batches) sum X^T X, n = 1 for a 2-D input
    and the leading dimension otherwise; the host count follows the device count without reading it back."""
    gen = torch.Generator().manual_seed(3)
    m = nn.Sequential(nn.Linear(32, 8, bias=True))
    w, bias = m[0].weight.detach().clone(), m[0].bias.detach().clone()
    quantize_(m, GPTQConfig("observe", Int8WeightOnlyConfig()))
    xs = [torch.randn(5, 32, generator=gen), torch.randn(3, 4, 32, generator=gen), torch.randn(7, 32, generator=gen)]
    want, tb = np.zeros((32, 32)), 0
    for x in xs:
        y = m(x)
        assert torch.equal(y, torch.nn.functional.linear(x, w, bias))
        n = 1 if x.dim() == 2 else x.shape[0]
        x2 = x.reshape(-1, 32).double().numpy()
        want = want * (tb / (tb + n)) + (2.0 / (tb + n)) * (x2.T @ x2)
        tb += n
    obs = m[0].weight
    assert obs.batches == 5 and obs.total_batches.tolist() == [5] and obs.hessian.dtype == torch.float32
    np.testing.assert_allclose(obs.hessian.numpy(), want, rtol=0, atol=1e-5 * np.abs(want).max())
    rebuilt = GPTQObserverTensor(obs.hp_data, obs.total_batches, obs.hessian)  # the count is read back once
    assert rebuilt.batches == 5


def test_int8_has_no_group_rule():
    """int8 per row has no quantization group: K and the block need only be multiples of 16, so a K that the block size does not divide
    (K = 192 with B = 128, K = 2000 or 320 with B = 256) passes the shape rules of the entry and of gptq_quantize alike.  With a null W
    the entry gets past them to its pointer check, and launches nothing."""
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    for K, k0, bw in ((2000, 0, 256), (2000, 1792, 208), (192, 0, 128), (192, 128, 64), (320, 256, 64)):
        assert lib.ao_gptq_block(None, 1, one, one, 1, 0, one, None, None, one, 4, K, k0, bw, None) == _lib.AO_ERR_NULL_POINTER, (K, k0, bw)
    assert lib.ao_gptq_block(None, 1, one, one, 1, 0, one, None, None, one, 4, 2000, 8, 256, None) == _lib.AO_ERR_INVALID_ARGUMENT  # k0 % 16
    assert lib.ao_gptq_block(None, 1, one, one, 0, 128, one, one, one, None, 4, 192, 0, 128, None) == _lib.AO_ERR_INVALID_ARGUMENT  # int4: K % g
    for K, B in ((192, 128), (2000, 256), (320, 256)):
        with pytest.raises(RuntimeError, match="expected the weight on the GPU"):  # every shape rule passed
            gptq_quantize(torch.eye(K), torch.zeros(16, K, dtype=torch.bfloat16), GPTQConfig("convert", Int8WeightOnlyConfig(), gptq_quantize_block_size=B))


def test_every_entry_rule_is_checked_before_anything_is_consumed():
    """what ao_gptq_block would refuse, gptq_quantize refuses first, as ValueError, with H and W untouched"""
    H, W = torch.eye(192), torch.ones(16, 192, dtype=torch.bfloat16)
    H[3, 3] = 0  # a dead column: the first thing the call would change
    for base, B, frag in ((Int4WeightOnlyConfig(group_size=16), 128, "one of 32, 64, 128, 256"), (Int4WeightOnlyConfig(group_size=128), 128, "multiple of the group size"),
                          (Int8WeightOnlyConfig(), 24, "multiple of the group size 16"), (NVFP4DynamicActivationNVFP4WeightConfig(), 320, "larger than 256")):
        with pytest.raises(ValueError, match=frag):
            gptq_quantize(H, W, GPTQConfig("convert", base, gptq_quantize_block_size=B))
    with pytest.raises(ValueError, match="empty weight"):
        gptq_quantize(torch.eye(0), torch.zeros(16, 0, dtype=torch.bfloat16), GPTQConfig("convert", Int8WeightOnlyConfig()))
    assert H[3, 3] == 0 and torch.all(W == 1)
