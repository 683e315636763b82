"""CPU: SmoothQuant's restatement against the fixture recorded from the reference's observers and convert, the config, the refusals, the
observers' protocol on CPU tensors (the torch-op path onto the same state), and the entries' argument rules.  No kernel runs here."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import smoothquant_cases as C
import smoothquant_ref as R
from ao_amd import _lib, ops, prototype
from ao_amd.prototype.nvfp4_tensor import QuantizationStep
from ao_amd.prototype.smoothquant import (
    RunningAbsMaxSmoothQuantObserver,
    SmoothQuantConfig,
    SmoothQuantObservedLinear,
    SmoothQuantObserver,
    SmoothQuantStep,
)
from ao_amd.quantization import quantize_
from ao_amd.quantization.config import (
    Float8DynamicActivationFloat8WeightConfig,
    Int4WeightOnlyConfig,
    Int8DynamicActivationInt8WeightConfig,
    Int8StaticActivationInt8WeightConfig,
    Int8WeightOnlyConfig,
    config_from_dict,
    config_to_dict,
)
from ao_amd.quantization.granularity import PerRow, PerTensor
from ao_amd.quantization.quant_primitives import MappingType
from oracle import bf16

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smoothquant.npz"))
META = json.loads(str(GOLDEN["meta"]))
DYN = Int8DynamicActivationInt8WeightConfig()
STATIC = Int8StaticActivationInt8WeightConfig(granularity=PerTensor())
INV, NULL, OK = _lib.AO_ERR_INVALID_ARGUMENT, _lib.AO_ERR_NULL_POINTER, _lib.AO_OK


def t16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16)


def golden_inputs():
    return [GOLDEN[f"x{i}"] for i in range(len(META["batches"]))]


# ---- the restatement against the reference's recorded results ------------------------------------------------------------------------------------
def test_restatement_of_the_absmax_equals_the_fixture():
    xs = golden_inputs()
    assert [x.shape[0] for x in xs] == META["batches"]
    state = None
    for x in xs:
        state = R.col_absmax(x, state)
    assert np.array_equal(bf16.to_bits(state), GOLDEN["x_abs_max"])
    assert np.array_equal(state, R.col_absmax(np.concatenate(xs)))  # folding over batches is the maximum of the concatenation
    assert np.array_equal(bf16.to_bits(R.col_absmax(GOLDEN["W"])), GOLDEN["w_abs_max"])
    assert (bf16.from_bits(GOLDEN["w_abs_max"]) == 0).any() and (bf16.from_bits(GOLDEN["x_abs_max"]) == 0).any()


@pytest.mark.parametrize("i", range(len(META["alphas"])), ids=[f"alpha={a}" for a in META["alphas"]])
def test_restatement_equals_the_fixture_byte_for_byte(i):
    alpha, p = META["alphas"][i], f"a{i}_"
    W, xs = GOLDEN["W"], golden_inputs()
    s = R.smoothing_factor(bf16.from_bits(GOLDEN["x_abs_max"]), bf16.from_bits(GOLDEN["w_abs_max"]), alpha)
    assert np.array_equal(bf16.to_bits(s), GOLDEN[p + "sf_bits"])
    if alpha is None:
        assert np.all(s == 1)
    assert np.array_equal(bf16.to_bits(R.pre_scale(s)), GOLDEN[p + "pre_bits"])
    Ws = R.smoothed_weight(W, s)
    q, sc = R.quantize_weight(Ws)
    assert np.array_equal(q, GOLDEN[p + "dyn_qdata"]) and np.array_equal(sc, GOLDEN[p + "dyn_scale"].reshape(-1))
    q, sc = R.quantize_weight(Ws, per_tensor=True)
    assert np.array_equal(q, GOLDEN[p + "static_qdata"]) and sc == GOLDEN[p + "static_scale"].reshape(())
    amax = np.float32(0)
    for x in xs:
        amax = R.smoothed_amax(x, s, amax)
    assert amax == np.abs(bf16.div(np.concatenate(xs), s[None, :])).max()
    assert R.static_scale(amax) == GOLDEN[p + "static_act_scale"].reshape(())
    assert R.running_scale(amax) == GOLDEN[p + "running_act_scale"].reshape(())


def test_restatement_of_the_prescaled_casts_rounds_the_product_once():
    """the halfway product 1.5 (1 + 2^-7) goes to the even neighbour; a row's amax moves to the column the pre-scale lifts"""
    x, pre = C.activation(12, 104, 3), C.pre_scale(104, 3)
    t = R.prescaled(x, pre)
    assert pre[0] == 1.5 and abs(x[0, 0]) == C.TIE and abs(t[0, 0]) == np.float32(1.515625)  # 1.51171875 is the tie; 1.515625 has the even code
    r = 1  # r % 5 == 1
    assert np.argmax(np.abs(x[r])) % 97 == 2 and np.argmax(np.abs(t[r])) % 97 == 3
    q, s = R.quantize_rowwise_prescaled(x, pre)
    q2, s2 = R.quantize_tensorwise_prescaled(x, pre)
    assert q.dtype == np.int8 and s.shape == (12,) and np.float32(s2) == s.max() and np.array_equal(q2[np.argmax(s)], q[np.argmax(s)])
    assert np.array_equal(R.quantize_static_prescaled(x, pre, [0.25]), R.quantize_static(t, [0.25]))


# ---- the config ------------------------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_step_parsing():
    c = SmoothQuantConfig(DYN, step="prepare")
    assert c.alpha == 0.5 and c.use_running_absmax is False and c.base_config is DYN and c.step == "prepare"
    assert SmoothQuantConfig(DYN, step="CONVERT").step == SmoothQuantStep.CONVERT == QuantizationStep.CONVERT
    assert SmoothQuantConfig(DYN, QuantizationStep.PREPARE_FOR_LOADING).step == "prepare_for_loading"
    assert SmoothQuantConfig(DYN, SmoothQuantStep.PREPARE_FOR_SMOOTHQUANT_SMOOTHING_FACTOR).step == "prepare_for_smoothquant_smoothing_factor"
    assert SmoothQuantConfig(DYN, "Prepare_For_SmoothQuant_Activation_Scales").step == "prepare_for_smoothquant_activation_scales"
    assert [s.value for s in SmoothQuantStep] == ["prepare", "convert", "prepare_for_loading", "prepare_for_smoothquant_smoothing_factor",
                                                  "prepare_for_smoothquant_activation_scales"]
    with pytest.raises(ValueError, match=r"calibrate is not one of \['prepare', 'convert', 'prepare_for_loading', "
                                         r"'prepare_for_smoothquant_smoothing_factor', 'prepare_for_smoothquant_activation_scales'\]"):
        SmoothQuantConfig(DYN, step="calibrate")


def test_quantization_step_keeps_its_three_members():
    assert [s.value for s in QuantizationStep] == ["prepare", "convert", "prepare_for_loading"]


def test_config_round_trip():
    c = SmoothQuantConfig(Int8StaticActivationInt8WeightConfig(granularity=[PerTensor(), PerRow()]), step="convert", alpha=0.75, use_running_absmax=True)
    d = json.loads(json.dumps(config_to_dict(c)))
    assert d["_type"] == "SmoothQuantConfig" and d["_data"]["base_config"]["_type"] == "Int8StaticActivationInt8WeightConfig"
    back = config_from_dict(d)
    assert back == c and back.alpha == 0.75 and back.use_running_absmax is True


def test_exports():
    for name in ("sq_col_absmax_update", "sq_smoothed_amax_update", "int8_quantize_rowwise_prescaled", "int8_quantize_tensorwise_prescaled",
                 "int8_quantize_static_prescaled", "int8_linear_prescaled", "int8_linear_tensorwise_prescaled", "int8_linear_static_prescaled"):
        assert name in ops.__all__
    for name in ("SmoothQuantConfig", "SmoothQuantStep", "SmoothQuantObserver", "RunningAbsMaxSmoothQuantObserver", "SmoothQuantObservedLinear"):
        assert name in prototype.__all__ and getattr(prototype, name) is getattr(prototype.smoothquant, name)
    for name in ENTRIES:
        assert name in _lib.declared_symbols() and name in _lib._SIGNATURES
    for name in ("int8_linear_prescaled", "int8_linear_tensorwise_prescaled", "int8_linear_static_prescaled"):
        assert hasattr(torch.ops.ao_mi355, name)


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------------------
REFUSED = [
    (Int8StaticActivationInt8WeightConfig(), "static PerRow activation"),
    (Int8StaticActivationInt8WeightConfig(granularity=[PerRow(), PerTensor()]), "static PerRow activation"),
    (Int8StaticActivationInt8WeightConfig(granularity=PerTensor(), act_mapping_type=MappingType.ASYMMETRIC), "static ASYMMETRIC activation"),
    (Int8WeightOnlyConfig(), "unsupported base_config Int8WeightOnlyConfig"),
    (Int4WeightOnlyConfig(group_size=32), "unsupported base_config Int4WeightOnlyConfig"),
    (Float8DynamicActivationFloat8WeightConfig(), "unsupported base_config Float8DynamicActivationFloat8WeightConfig"),
]


@pytest.mark.parametrize("base,frag", REFUSED, ids=[f"{type(b).__name__}-{i}" for i, (b, _) in enumerate(REFUSED)])
def test_unsupported_bases_are_refused_by_name_at_prepare(base, frag):
    m = nn.Sequential(nn.Linear(64, 16, bias=False)).to(torch.bfloat16)
    for step in ("prepare", "prepare_for_loading"):
        with pytest.raises(NotImplementedError, match=frag) as e:
            quantize_(m, SmoothQuantConfig(base, step=step))
        assert "SmoothQuant on MI355X supports" in str(e.value)
    assert type(m[0]) is nn.Linear


def test_unsupported_weights_are_refused_by_name_at_prepare():
    class ThreeD(nn.Module):
        def __init__(self):
            super().__init__()
            self.weight = nn.Parameter(torch.zeros(2, 16, 64, dtype=torch.bfloat16))

    cfg = SmoothQuantConfig(DYN, step="prepare")
    with pytest.raises(NotImplementedError, match=r"2-D weights, got shape \(2, 16, 64\)"):
        quantize_(ThreeD(), cfg, filter_fn=lambda m, fqn: isinstance(m, ThreeD))
    with pytest.raises(NotImplementedError, match="bfloat16 weights, got torch.float32"):
        quantize_(nn.Sequential(nn.Linear(64, 16)), cfg)
    with pytest.raises(NotImplementedError, match="bfloat16 weights, got torch.float16"):
        quantize_(nn.Sequential(nn.Linear(64, 16)).half(), cfg)
    with pytest.raises(NotImplementedError, match="K=60 is not a multiple of 8"):
        quantize_(nn.Sequential(nn.Linear(60, 16)).to(torch.bfloat16), cfg)


def test_supported_bases_prepare_and_unobserved_modules_are_skipped_at_convert(caplog):
    supported = [DYN, Int8DynamicActivationInt8WeightConfig(granularity=PerTensor()),
                 Int8DynamicActivationInt8WeightConfig(granularity=[PerTensor(), PerRow()]),
                 Int8DynamicActivationInt8WeightConfig(act_mapping_type=MappingType.ASYMMETRIC), STATIC,
                 Int8StaticActivationInt8WeightConfig(granularity=[PerTensor(), PerRow()])]
    for base in supported:
        for running in (False, True):
            m = nn.Sequential(nn.Linear(64, 16, bias=True)).to(torch.bfloat16)
            w, b = m[0].weight, m[0].bias
            quantize_(m, SmoothQuantConfig(base, step="prepare", use_running_absmax=running))
            assert isinstance(m[0], SmoothQuantObservedLinear) and m[0].weight is w and m[0].bias is b
            assert isinstance(m[0].obs, RunningAbsMaxSmoothQuantObserver if running else SmoothQuantObserver)
            if not running:
                assert m[0].obs.keep_inputs == isinstance(base, Int8StaticActivationInt8WeightConfig)
    plain = nn.Sequential(nn.Linear(64, 16)).to(torch.bfloat16)
    with caplog.at_level("INFO", logger="ao_amd.prototype.smoothquant.api"):
        quantize_(plain, SmoothQuantConfig(DYN, step="convert"))
    assert type(plain[0]) is nn.Linear and "convert: module is not SmoothQuantObservedLinear, skipping" in caplog.text
    for step in ("prepare_for_smoothquant_smoothing_factor", "prepare_for_smoothquant_activation_scales"):
        quantize_(plain, SmoothQuantConfig(DYN, step=step))
        assert type(plain[0]) is nn.Linear


# ---- the observers, on CPU tensors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [SmoothQuantObserver, RunningAbsMaxSmoothQuantObserver])
def test_calculate_qparams_before_calibration_raises(cls):
    obs = cls(t16(GOLDEN["W"]), 0.5)
    with pytest.raises(AssertionError, match="calibrate observer first by running model on exemplar data"):
        obs.calculate_qparams()
    if cls is RunningAbsMaxSmoothQuantObserver:
        with pytest.raises(AssertionError, match="calibrate observer first"):
            obs.compute_smoothing_factor()


@pytest.mark.parametrize("cls", [SmoothQuantObserver, RunningAbsMaxSmoothQuantObserver])
def test_alpha_none_gives_ones_and_the_input_comes_back_unchanged(cls):
    obs = cls(t16(GOLDEN["W"]), None)
    x = t16(GOLDEN["x0"])
    assert obs(x) is x
    sf, scale, zp = obs.calculate_qparams()
    assert sf.dtype == torch.bfloat16 and sf.shape == (META["K"],) and torch.all(sf == 1) and scale is None and zp is None


@pytest.mark.parametrize("i", range(len(META["alphas"])), ids=[f"alpha={a}" for a in META["alphas"]])
def test_observers_on_the_cpu_reach_the_fixtures_state(i):
    """the torch-op path: x_abs_max exactly; the smoothing factor is the reference's own ops on the same vectors, so here (same torch, same
    CPU) exactly too; the activation scales exactly"""
    alpha, p = META["alphas"][i], f"a{i}_"
    W, xs = t16(GOLDEN["W"]), [t16(x) for x in golden_inputs()]
    obs, run = SmoothQuantObserver(W, alpha), RunningAbsMaxSmoothQuantObserver(W, alpha)
    for n, x in enumerate(xs):
        obs(x.reshape(1, -1, META["K"]) if n == 0 else x)  # a 3-D input is flattened
        run(x)
    assert obs.calibration_count == run.calibration_count == 3 and isinstance(obs.calibration_count, int)
    for o in (obs, run):
        assert o.x_abs_max.dtype == torch.float32 and np.array_equal(bf16.to_bits(o.x_abs_max.numpy()), GOLDEN["x_abs_max"])
    assert np.array_equal(bf16.to_bits(obs.w_abs_max().float().numpy()), GOLDEN["w_abs_max"])
    kwargs = STATIC.get_act_quant_kwargs()
    sf, scale, zp = obs.calculate_qparams(kwargs)
    assert np.array_equal(bf16.to_bits(sf.float().numpy()), GOLDEN[p + "sf_bits"]) and zp is None
    assert scale.dtype == torch.float32 and scale.shape == (1, 1) and np.array_equal(scale.numpy(), GOLDEN[p + "static_act_scale"])
    assert run.calculate_qparams(kwargs)[1] is None  # no second pass yet (reference core.py:308-310)
    assert torch.equal(run.compute_smoothing_factor(), sf) and run._in_second_pass and run._second_pass_count == 0
    for x in xs:
        run(x)
    assert run._second_pass_count == 3 and run.calibration_count == 3
    for kw in (kwargs, {"quant_min": -128, "quant_max": 127, "qscheme": torch.per_tensor_symmetric}):
        sf_r, scale_r, zp_r = run.calculate_qparams(kw)
        assert torch.equal(sf_r, sf) and zp_r is None and scale_r.dtype == torch.float32 and scale_r.shape == ()
        assert scale_r.numpy() == GOLDEN[p + "running_act_scale"].reshape(())
    run.compute_smoothing_factor()  # again: the second pass starts over
    assert run._second_pass_count == 0 and run._smooth_amax is None
    run(xs[0])
    with pytest.raises(NotImplementedError, match="symmetric"):
        run.calculate_qparams({"quant_min": -128, "quant_max": 127, "is_symmetric": False})
    with pytest.raises(NotImplementedError, match="PerTensor symmetric"):
        obs.calculate_qparams(Int8StaticActivationInt8WeightConfig().get_act_quant_kwargs())


def test_observer_without_kept_inputs_keeps_only_the_running_maximum():
    obs = SmoothQuantObserver(t16(GOLDEN["W"]), 0.5, keep_inputs=False)
    for x in golden_inputs():
        obs(t16(x))
    assert obs.inputs == [] and np.array_equal(bf16.to_bits(obs.x_abs_max.numpy()), GOLDEN["x_abs_max"])
    assert np.array_equal(bf16.to_bits(obs.calculate_qparams()[0].float().numpy()), GOLDEN["a3_sf_bits"])
    with pytest.raises(AssertionError, match="kept no inputs"):
        obs.calculate_qparams(STATIC.get_act_quant_kwargs())


# ---- the entries' argument rules (no launch) ---------------------------------------------------------------------------------------------------
def _entries():
    lib = _lib.lib()
    return {
        "ao_sq_col_absmax_update": lambda M, K: lib.ao_sq_col_absmax_update(None, None, M, K, None),
        "ao_sq_smoothed_amax_update": lambda M, K: lib.ao_sq_smoothed_amax_update(None, None, None, M, K, None),
        "ao_int8_quantize_rowwise_prescaled": lambda M, K: lib.ao_int8_quantize_rowwise_prescaled(None, None, None, None, M, K, None),
        "ao_int8_quantize_tensorwise_prescaled": lambda M, K: lib.ao_int8_quantize_tensorwise_prescaled(None, None, None, None, None, M, K, None),
        "ao_int8_quantize_static_prescaled": lambda M, K: lib.ao_int8_quantize_static_prescaled(None, None, None, None, 0, None, M, K, None),
    }


ENTRIES = ["ao_sq_col_absmax_update", "ao_sq_smoothed_amax_update", "ao_int8_quantize_rowwise_prescaled",
           "ao_int8_quantize_tensorwise_prescaled", "ao_int8_quantize_static_prescaled"]


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_validate_on_the_host(name):
    call = _entries()[name]
    assert call(0, 64) == OK  # no rows: no launch, no pointer is looked at, no GPU is needed
    for M, K, reason in [(4, 12, "K=12 must be a multiple of 8"), (4, 0, "bad shape M=4 K=0"), (-1, 64, "bad shape M=-1 K=64"),
                         (1 << 31, 64, "too large")]:
        assert call(M, K) == INV and reason in _lib.last_error() and _lib.last_error().startswith(name + ":"), (M, K, _lib.last_error())
        with pytest.raises(ValueError):
            _lib.check(call(M, K))
    # null pointers are refused by name before anything is launched (the library's null-pointer code, an invalid argument by another name)
    assert call(4, 64) == NULL and "null pointer argument 'x'" in _lib.last_error() and _lib.last_error().startswith(name + ":")


def test_wrappers_refuse_what_the_kernels_do_not_take():
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="expected all tensors on the GPU"):
        ops.sq_col_absmax_update(x, torch.zeros(64))
    with pytest.raises(RuntimeError, match="expected all tensors on the GPU"):
        ops.int8_quantize_rowwise_prescaled(x, torch.ones(64, dtype=torch.bfloat16))
