"""CPU: float8 training -- the numpy restatement of the training cast against the fixture written from the reference
(tests/golden/fp8_training.npz), byte for byte; the config mirror against the reference's recorded fields; every refusal with its reason
and no GPU; model conversion; the C entry points' argument checks (no kernel is launched in this file)."""
import ctypes
import dataclasses
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import fp8_training_ref as R
from ao_amd import _lib, float8 as F8, ops
from ao_amd.float8 import CastConfig, Float8LinearConfig, Float8LinearRecipeName, ScalingGranularity, ScalingType, e4m3_dtype, e5m2_dtype
from ao_amd.float8.float8_linear import Float8Linear, LinearMMConfig, check_config, matmul_with_hp_or_float8_args
from ao_amd.float8.float8_linear_utils import convert_to_float8_training, swap_linear_layers

HERE = os.path.dirname(os.path.abspath(__file__))
E4M3_TENSORWISE = Float8LinearConfig(cast_config_grad_output=CastConfig(target_dtype=e4m3_dtype))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MAKER = _load("make_golden_fp8_training")


@functools.lru_cache(maxsize=None)
def fixture():
    return MAKER.load()


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


CASTS = [(t, tag, ax, p) for t in ("x", "go", "w", "edge") for tag, ax in MAKER.AXES for p in (0, 1)]


# ---- the cast ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,tag,ax,p", CASTS, ids=["%s_%s%d" % (t, tag, p) for t, tag, ax, p in CASTS])
def test_the_restatement_reproduces_every_recorded_cast(t, tag, ax, p):
    G = fixture()
    xb = G[t].reshape(-1, G[t].shape[-1])
    q, s, inv = R.cast(xb, ax, bool(p))
    key = "%s_%s%d" % (t, tag, p)
    assert G[key + "_q"].shape == xb.shape and G[key + "_s"].dtype == np.float32
    np.testing.assert_array_equal(q, G[key + "_q"])
    np.testing.assert_array_equal(_u32(s).reshape(G[key + "_s"].shape), _u32(G[key + "_s"]))
    np.testing.assert_array_equal(_u32(inv), _u32(1.0 / torch.from_numpy(np.asarray(s, dtype=np.float32).copy())))  # torch.reciprocal


def test_every_recorded_power_of_two_scale_is_the_plain_scale_with_its_mantissa_cleared():
    G = fixture()
    n = 0
    for t, tag, ax, p in CASTS:
        if p:
            plain, rounded = G["%s_%s0_s" % (t, tag)], G["%s_%s1_s" % (t, tag)]
            np.testing.assert_array_equal(_u32(rounded), _u32(R.clear_mantissa(plain)))
            assert np.all((_u32(rounded) & 0x7FFFFF) == 0) and np.all(rounded <= plain) and np.all(rounded * 2 > plain)
            n += 1
    assert n == 12


def test_the_edge_tensor_holds_its_edge_cases():
    G = fixture()
    e = R.bf16.from_bits(G["edge"])
    assert not e[3].any() and not e[:, 5].any() and e[7, 11] == np.float32(torch.finfo(torch.bfloat16).max) and 0 < e[20, 9] < 1e-19
    assert G["edge_r0_s"][3, 0] == np.float32(448.0 / 1e-12) and not G["edge_r0_q"][3].any()  # the zero row: amax clamped to 1e-12
    assert G["edge_r0_q"][7, 11] == 0x7E  # the largest bf16 lands on 448
    # the clamp is live: without the power-of-two rounding some amax * scale rounds above 448
    x = R.bf16.from_bits(G["x"].reshape(-1, G["x"].shape[-1])).astype(np.float32)
    assert np.any(np.abs(x * G["x_r0_s"]) > 448.0) or np.any(np.abs(x * G["x_c0_s"]) > 448.0)


# ---- the config mirror ---------------------------------------------------------------------------------------------------------------
def test_from_recipe_name_has_the_recorded_fields():
    rec = json.loads(str(fixture()["recipes"]))
    assert sorted(rec) == sorted(n.value for n in Float8LinearRecipeName)
    for name in Float8LinearRecipeName:
        assert MAKER.config_fields(Float8LinearConfig.from_recipe_name(name)) == rec[name.value], name
        assert Float8LinearConfig.from_recipe_name(name.value) == Float8LinearConfig.from_recipe_name(name)  # string names are accepted
    with pytest.raises(AssertionError, match="not in valid names"):
        Float8LinearConfig.from_recipe_name("blockwise")


def test_post_init_fills_in_the_second_configs_and_rejects_a_mixed_gemm():
    c = Float8LinearConfig()
    assert c.cast_config_input_for_grad_weight is c.cast_config_input and c.cast_config_weight_for_grad_input is c.cast_config_weight
    assert c.cast_config_grad_output_for_grad_weight is c.cast_config_grad_output
    assert c.cast_config_input.target_dtype == e4m3_dtype == torch.float8_e4m3fn and c.cast_config_weight.target_dtype == e4m3_dtype
    assert c.cast_config_grad_output.target_dtype == e5m2_dtype == torch.float8_e5m2
    assert c.gemm_config_output.use_fast_accum and not c.gemm_config_grad_input.use_fast_accum and not c.round_scales_to_power_of_2
    with pytest.raises(dataclasses.FrozenInstanceError):
        c.emulate = True
    with pytest.raises(AssertionError, match="incompatible operand precision for output"):
        Float8LinearConfig(cast_config_input=CastConfig(scaling_type=ScalingType.DISABLED))
    with pytest.raises(AssertionError, match="same dtype in both matmuls"):
        Float8LinearConfig(cast_config_input=CastConfig(target_dtype=e4m3_dtype), cast_config_input_for_grad_weight=CastConfig(target_dtype=e5m2_dtype))
    with pytest.raises(AssertionError, match="only dynamic scaling"):
        CastConfig(scaling_type=ScalingType.DISABLED, scaling_granularity=ScalingGranularity.AXISWISE)
    with pytest.raises(AssertionError, match="8-bit floating-point"):
        CastConfig(target_dtype=torch.bfloat16)
    with pytest.raises(AssertionError, match="tensorwise scaling granularity"):
        Float8LinearConfig(cast_config_weight=CastConfig(scaling_granularity=ScalingGranularity.AXISWISE), enable_fsdp_float8_all_gather=True)
    assert CastConfig(target_dtype=e4m3_dtype).short_str() == "dyn_ten_e4m3"
    assert CastConfig(scaling_type=ScalingType.DISABLED, target_dtype=e5m2_dtype).short_str() == "dis_ten_e5m2"
    assert set(F8.__all__) >= {"ScalingType", "ScalingGranularity", "Float8GemmConfig", "Float8LinearConfig", "Float8LinearRecipeName",
                               "CastConfig", "convert_to_float8_training"}


# ---- refusals, each before any GPU requirement -----------------------------------------------------------------------------------------
def _lin(k=32, n=16, **kw):
    return nn.Linear(k, n, **kw).to(torch.bfloat16)


@pytest.mark.parametrize("config", [Float8LinearConfig(), Float8LinearConfig.from_recipe_name("tensorwise"), None], ids=["default", "recipe", "none"])
def test_an_e5m2_grad_output_is_refused_with_the_working_alternative(config):
    for call in (lambda: convert_to_float8_training(nn.Sequential(_lin()), config=config), lambda: Float8Linear.from_float(_lin(), config),
                 lambda: Float8Linear(32, 16, config=config or Float8LinearConfig())):
        with pytest.raises(ValueError, match=r"float8_e5m2.*Float8LinearConfig\(cast_config_grad_output=CastConfig\(target_dtype=e4m3_dtype\)\)"):
            call()
    check_config(E4M3_TENSORWISE)  # the alternative the message names is accepted


def test_fsdp_all_gather_and_pad_inner_dim_are_refused():
    with pytest.raises(ValueError, match="enable_fsdp_float8_all_gather"):
        Float8Linear.from_float(_lin(), dataclasses.replace(E4M3_TENSORWISE, enable_fsdp_float8_all_gather=True))
    with pytest.raises(ValueError, match="pad_inner_dim"):
        convert_to_float8_training(_lin(), config=dataclasses.replace(Float8LinearConfig.from_recipe_name("rowwise"), pad_inner_dim=True))
    with pytest.raises(AssertionError, match="Float8LinearConfig"):
        check_config("rowwise")


def _apply(x, w, config):
    return matmul_with_hp_or_float8_args.apply(x, w.t(), LinearMMConfig(), config)


def test_operands_that_the_function_does_not_take_are_refused_on_the_cpu():
    rw, hp = Float8LinearConfig.from_recipe_name("rowwise"), Float8LinearConfig.from_recipe_name("rowwise_with_gw_hp")
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)  # noqa: E731
    with pytest.raises(AssertionError, match="input must be bfloat16"):
        _apply(torch.zeros(16, 32), bf(16, 32), rw)
    with pytest.raises(AssertionError, match="weight must be bfloat16"):
        _apply(bf(16, 32), torch.zeros(16, 32, dtype=torch.float16), rw)
    with pytest.raises(AssertionError, match="already cast to float8"):
        _apply(bf(16, 32).to(torch.float8_e4m3fn), bf(16, 32), rw)
    with pytest.raises(AssertionError, match="K and N must be multiples of 16.*K=24"):
        _apply(bf(16, 24), bf(16, 24), rw)
    with pytest.raises(AssertionError, match="K and N must be multiples of 16.*N=24"):
        _apply(bf(16, 32), bf(24, 32), rw)
    with pytest.raises(AssertionError, match="not compatible"):
        _apply(bf(16, 32), bf(16, 48), rw)
    with pytest.raises(AssertionError, match="M=24 tokens must be a multiple of 16.*ROWWISE_WITH_GW_HP.*freeze the weight"):
        _apply(bf(2, 12, 32), bf(16, 32).requires_grad_(True), rw)
    # M = 24 passes the checks where grad_weight is not a float8 GEMM, and fails only at the GPU requirement
    for w, cfg in ((bf(16, 32).requires_grad_(True), hp), (bf(16, 32), rw)):
        with pytest.raises(RuntimeError, match="expected all tensors on the GPU"):
            _apply(bf(2, 12, 32), w, cfg)
    with pytest.raises(ValueError, match="float8_e5m2"):
        _apply(bf(16, 32), bf(16, 32), Float8LinearConfig())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Float8Linear.from_float(_lin(), rw)(bf(16, 32))


def test_the_ops_refuse_shapes_and_tensors_on_the_cpu():
    x = torch.zeros(16, 32, dtype=torch.bfloat16)
    for name in ("fp8_train_amax", "fp8_train_cast", "fp8_train_quantize_rowwise", "fp8_train_quantize_colwise_t", "fp8_train_quantize_both"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    for fn in (ops.fp8_train_amax, ops.fp8_train_quantize_rowwise, ops.fp8_train_quantize_colwise_t, ops.fp8_train_quantize_both):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)


# ---- model conversion --------------------------------------------------------------------------------------------------------------------
class Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.up = nn.Linear(32, 64, bias=True)
        self.act = nn.GELU()
        self.down = nn.Linear(64, 32, bias=False)


def _model():
    return nn.Sequential(nn.ModuleDict({"a": Block(), "b": Block()}), nn.LayerNorm(32), nn.Linear(32, 16)).to(torch.bfloat16)


def test_convert_swaps_exactly_the_linears_the_filter_passes():
    cfg = Float8LinearConfig.from_recipe_name("rowwise")
    model = _model()
    before = dict(model.named_parameters())
    seen = []

    def keep(mod, fqn):
        assert isinstance(mod, nn.Linear)  # the filter is asked about linears only
        seen.append(fqn)
        return "down" not in fqn and fqn != "2"

    out = convert_to_float8_training(model, module_filter_fn=keep, config=cfg)
    assert out is model
    assert seen == ["0.a.up", "0.a.down", "0.b.up", "0.b.down", "2"]  # post-order: children before their parent, in definition order
    kinds = {n: type(m) for n, m in model.named_modules() if isinstance(m, nn.Linear)}
    assert kinds == {"0.a.up": Float8Linear, "0.a.down": nn.Linear, "0.b.up": Float8Linear, "0.b.down": nn.Linear, "2": nn.Linear}
    after = dict(model.named_parameters())
    assert after.keys() == before.keys() and all(after[k] is before[k] for k in before)  # weight and bias are the same Parameter objects
    up = model[0]["a"].up
    assert up.config is cfg and up.in_features == 32 and up.out_features == 64 and up.bias is not None
    assert up.linear_mm_config.output.use_fast_accum and not up.linear_mm_config.grad_input.use_fast_accum
    assert up.scaling_type_input is ScalingType.DYNAMIC
    # no filter: every linear
    model = convert_to_float8_training(_model(), config=cfg)
    assert all(type(m) is Float8Linear for m in model.modules() if isinstance(m, nn.Linear))


def test_a_root_linear_is_returned_not_modified():
    cfg = Float8LinearConfig.from_recipe_name("rowwise")
    lin = _lin(bias=True)
    out = convert_to_float8_training(lin, config=cfg)
    assert type(lin) is nn.Linear and type(out) is Float8Linear and out is not lin
    assert out.weight is lin.weight and out.bias is lin.bias
    assert convert_to_float8_training(lin, config=cfg, module_filter_fn=lambda m, fqn: False) is lin
    assert swap_linear_layers(lin, lambda m: "swapped") == "swapped"


@pytest.mark.parametrize("name,want", [
    ("rowwise", "i:dyn_axs_e4m3,w:dyn_axs_e4m3,go:dyn_axs_e4m3"),
    ("rowwise_with_gw_hp", "i:dyn_axs_e4m3,w:dyn_axs_e4m3,go:dyn_axs_e4m3,i_gw:dis_ten_e4m3,w_gi:dyn_ten_e4m3,go_gw:dis_ten_e4m3"),
    ("tensorwise_e4m3", "i:dyn_ten_e4m3,w:dyn_ten_e4m3,go:dyn_ten_e4m3"),
])
def test_extra_repr_prints_the_references_string(name, want):
    cfg = E4M3_TENSORWISE if name == "tensorwise_e4m3" else Float8LinearConfig.from_recipe_name(name)
    m = Float8Linear.from_float(_lin(bias=False), cfg)
    assert m.extra_repr() == f'in_features=32, out_features=16, bias=False, cast_configs={want}"'


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_and_exported():
    names = _lib.declared_symbols()
    for n in ("ao_fp8_train_amax", "ao_fp8_train_cast", "ao_fp8_train_quantize_rowwise"):
        assert n in names and n in _lib._SIGNATURES and hasattr(_lib.lib(), n)
    text = open(_lib.HEADER_PATH).read()
    for cite in ("float8_utils.py:31-53", "float8_utils.py:244-246", "float8_training_tensor.py:153-154", "float8_utils.py:118-139", "float8_ops.py:44-45"):
        assert cite in text, cite


def test_the_entry_points_check_their_arguments_on_the_host():
    lib = _lib.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first, and an empty matrix launches nothing
    inv, ok = _lib.AO_ERR_INVALID_ARGUMENT, _lib.AO_OK
    cast = lambda r, c, qt=one: lib.ao_fp8_train_cast(one, one, 1, one, 1, 0, one, one, one, qt, one, one, r, c, None)  # noqa: E731
    assert lib.ao_fp8_train_amax(one, one, one, 16, 24, None) == inv and "C=24 must be a multiple of 16" in _lib.last_error()
    assert cast(16, 24) == inv and "C=24" in _lib.last_error()
    assert lib.ao_fp8_train_quantize_rowwise(one, one, one, one, 0, 16, 24, None) == inv and "C=24" in _lib.last_error()
    assert cast(24, 32) == inv and "R=24 must be a multiple of 16 for the transposed output" in _lib.last_error()
    assert lib.ao_fp8_train_cast(one, one, 2, one, 1, 0, one, one, one, one, one, one, 16, 32, None) == inv and "stride" in _lib.last_error()
    for r, c in ((0, 32), (16, 0), (0, 0)):
        assert lib.ao_fp8_train_amax(one, one, one, r, c, None) == ok
        assert cast(r, c) == ok
        assert lib.ao_fp8_train_quantize_rowwise(one, one, one, one, 1, r, c, None) == ok
    assert cast(0, 24) == inv  # the shape is checked before the matrix is found empty
    assert lib.ao_fp8_train_amax(None, one, one, 16, 32, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_fp8_train_amax(one, None, None, 16, 32, None) == inv and "neither" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(cast(24, 32))
