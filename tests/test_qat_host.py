"""Quantization-aware training without a GPU: the CPU restatement (tests/qat_ref.py) against the reference's recorded bytes
(tests/golden/qat.npz), the backward formulas against the reference's own int4 gradient and against float64 autograd, the configs and
their refusals, the module swaps of quantize_(QATConfig), and the C entries' host validation."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qat_ref as R  # noqa: E402
from ao_amd import _lib, ops  # noqa: E402
from ao_amd.quantization import (
    Float8DynamicActivationFloat8WeightConfig,
    Float8DynamicActivationInt4WeightConfig,
    Int4WeightOnlyConfig,
    Int8WeightOnlyConfig,
    PerBlock,
    PerGroup,
    PerRow,
    PerTensor,
    quantize_,
)
from ao_amd.quantization import qat
from ao_amd.quantization.qat import (
    FakeQuantizedLinear,
    FakeQuantizerBase,
    Float8FakeQuantizeConfig,
    Float8FakeQuantizer,
    Int4WeightFakeQuantizeConfig,
    Int4WeightFakeQuantizer,
    QATConfig,
    QATStep,
)
from ao_amd.quantization.qat.fake_quantize_config import _infer_fake_quantize_configs

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qat.npz"))
INT4_CASES = [tuple(int(v) for v in c) for c in GOLD["int4_cases"]]
FP8_NAMES = [str(n) for n in GOLD["fp8_names"]]


def fp8_case(name):
    lb, ub = (None if math.isnan(v) else float(v) for v in GOLD[f"fp8_{name}_cfg"])
    return R.from_bits(GOLD[f"fp8_{name}_x"]), lb, ub


# ---- the restatement against the fixture ------------------------------------------------------------------------------------------------
def test_fixture_holds_the_whole_grid():
    assert INT4_CASES == [(g, n, k) for g in (32, 64, 128, 256) for n, k in ((1, g), (3, 3 * g), (17, 5 * g))]
    assert set(FP8_NAMES) >= {f"r{r}c{c}" for c in (16, 48, 512, 1040, 8208) for r in (1, 3, 67)} | {"b2x5x48_0"}
    assert tuple(GOLD["fp8_b2x5x48_0_x"].shape) == (2, 5, 48)


@pytest.mark.parametrize("g,n,k", INT4_CASES)
def test_int4_restatement_forward_is_the_references_bytes(g, n, k):
    w = R.from_bits(GOLD[f"int4_g{g}_{n}x{k}_w"])
    assert np.array_equal(R.bits(R.int4_fake_quantize(w, g)), GOLD[f"int4_g{g}_{n}x{k}_out"])


@pytest.mark.parametrize("name", FP8_NAMES)
def test_fp8_restatement_forward_is_the_references_bytes(name):
    x, lb, ub = fp8_case(name)
    assert np.array_equal(R.bits(R.fp8_fake_quantize(x, lb, ub)), GOLD[f"fp8_{name}_out"])


def test_fp8_fixture_holds_its_planted_rows():
    seen_nan = seen_below = seen_above = False
    for name in FP8_NAMES:
        x, lb, ub = fp8_case(name)
        x2 = x.float().reshape(-1, x.shape[-1])
        amax = x2.abs().amax(-1)
        assert int((x2[0].abs() == amax[0]).sum()) == 2 and float(x2[0][x2[0].abs() == amax[0]].sum()) == 0.0  # the +- tie
        out = R.from_bits(GOLD[f"fp8_{name}_out"]).float().reshape(x2.shape)
        seen_nan |= bool(out.isnan().any())
        seen_below |= lb is not None and bool((amax < lb).any())
        seen_above |= ub is not None and bool((amax > ub).any())
        if lb is not None:
            assert not out.isnan().any()
    assert seen_nan and seen_below and seen_above


@pytest.mark.parametrize("g,n,k", INT4_CASES)
def test_references_int4_gradient_lies_inside_the_bound_of_the_formula(g, n, k):
    name = f"int4_g{g}_{n}x{k}"
    w, go, gw = (R.from_bits(GOLD[f"{name}_{s}"]) for s in ("w", "go", "gw"))
    want, mag = R.int4_fake_quantize_bwd(w, go, g)
    assert bool(((gw.double() - want).abs() <= R.bound(want, mag)).all())
    # the planted ties: the formula leaves the bound around G there, so the bound cannot hide a dropped range term
    x = w.float()[0, :g]
    for cols, value in ((GOLD["tie_max"], x.max()), (GOLD["tie_min"], x.min())):
        for c in cols:
            c = int(c) % g
            assert float(x[c]) == float(value)
            assert abs(float(want[0, c]) - float(go[0, c])) > float(R.bound(want, mag)[0, c])


def _fp8_chain_float64_autograd(x, go, lb, ub):
    """float64 autograd of the chain with every cast straight-through: the scale's bf16 rounding and the e4m3 rounding keep the forward's
    values and pass the gradient as the identity"""
    x32, amax32, inside, s32, t32, q32 = R._fp8_parts(x, lb, ub)
    xd = x32.double().requires_grad_()
    a = xd.abs().amax(-1, keepdim=True)
    lo, hi = R._bf16_bound(lb, -math.inf).double(), R._bf16_bound(ub, math.inf).double()
    a = torch.clamp(a, min=lo, max=hi)
    s_exact = a / 448
    s = s_exact + (s32.double() - s_exact).detach()
    t = xd / s
    tc = t.clamp(-448, 448)
    q = tc + (q32.double() - tc).detach()
    (q * s).backward(go.double().reshape(x32.shape))
    return xd.grad


@pytest.mark.parametrize("name", FP8_NAMES)
def test_fp8_formula_is_float64_autograd_with_straight_through_casts(name):
    x, lb, ub = fp8_case(name)
    gen = torch.Generator().manual_seed(5)
    go = (torch.randn(x.shape, generator=gen) * 1e-3).to(torch.bfloat16)
    want, mag = R.fp8_fake_quantize_bwd(x, go, lb, ub)
    auto = _fp8_chain_float64_autograd(x, go, lb, ub).reshape(x.shape)
    finite = ~want.isnan()
    assert bool((auto.isnan() == want.isnan()).all())
    # the forward's t is fp32 and autograd's float64: 2^-24 on each of the row's terms (t <= 448 and da = ds / 448 cancel)
    assert bool(((auto - want).abs()[finite] <= (mag * 2.0 ** -22)[finite]).all())
    row0 = x.float().reshape(-1, x.shape[-1])[0]
    for c in (2, x.shape[-1] - 3):  # the planted +- tie takes the range term, half each, with its sign
        assert abs(float(row0[c])) == float(row0.abs().max())
    w0, m0, g0 = (t.reshape(-1, x.shape[-1])[0] for t in (want, mag, go.double()))
    inside = lb is None or float(row0.abs().max()) >= lb
    inside &= ub is None or float(row0.abs().max()) <= ub
    if inside and x.shape[-1] > 16:
        c0 = float(R._fp8_parts(x, lb, ub)[4][0, 2].abs() <= 448)  # (the scale's bf16 rounding can leave the maximum past the clamp)
        up, down = float(w0[2] - c0 * g0[2]), float(w0[-3] - c0 * g0[-3])
        assert up != 0.0 and up == pytest.approx(-down, rel=1e-9)


# ---- configs ----------------------------------------------------------------------------------------------------------------------------
def test_float8_config_validates_like_the_reference_and_refuses_by_name():
    c = Float8FakeQuantizeConfig()
    assert (c.dtype, c.granularity, c.hp_value_lb, c.hp_value_ub) == (torch.float8_e4m3fn, PerRow(), None, None)
    with pytest.raises(ValueError, match="torch.bfloat16 is not a float8 dtype"):
        Float8FakeQuantizeConfig(dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"Please specify the granularity object instead of the class, e.g. PerRow\(\) instead of PerRow"):
        Float8FakeQuantizeConfig(granularity=PerRow)
    with pytest.raises(ValueError, match="Expected PerRow or PerTensor granularity, got PerGroup"):
        Float8FakeQuantizeConfig(granularity=PerGroup(32))
    with pytest.raises(NotImplementedError, match=r"only torch.float8_e4m3fn is implemented"):
        Float8FakeQuantizeConfig(dtype=torch.float8_e5m2)
    with pytest.raises(NotImplementedError, match=r"only PerRow\(\)"):
        Float8FakeQuantizeConfig(granularity=PerTensor())
    with pytest.raises(NotImplementedError, match=r"blockwise float8 fake quantization is not implemented.*use PerRow\(\)"):
        Float8FakeQuantizeConfig(granularity=PerBlock((1, 128)))


def test_int4_config_validates_like_the_reference_and_refuses_by_name():
    c = Int4WeightFakeQuantizeConfig()
    assert (c.group_size, c.activation_dtype) == (128, torch.bfloat16)
    with pytest.raises(ValueError, match="Only torch.float8_e4m3fn or torch.bfloat16 activation are supported"):
        Int4WeightFakeQuantizeConfig(activation_dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="use activation_dtype=torch.bfloat16"):
        Int4WeightFakeQuantizeConfig(activation_dtype=torch.float8_e4m3fn)


def test_qat_config_post_init_errors_word_for_word():
    base, fq = Int4WeightOnlyConfig(group_size=32), Int4WeightFakeQuantizeConfig(32)
    assert QATConfig(base).step == "prepare" == QATStep.PREPARE and QATConfig(base, step="CONVERT").step == QATStep.CONVERT
    assert QATConfig(step="convert").base_config is None

    def refused(message, *args, **kwargs):
        with pytest.raises(ValueError) as e:
            QATConfig(*args, **kwargs)
        assert str(e.value) == message

    refused("`step` must be one of ['prepare', 'convert']", base, step="train")
    refused("Cannot specify both `base_config` and `activation_config`", base, activation_config=Float8FakeQuantizeConfig())
    refused("Cannot specify both `base_config` and `weight_config`", base, weight_config=fq)
    refused("Must specify `base_config`, `activation_config`, or `weight_config` in the prepare step")
    refused("Cannot specify `weight_config` or `activation_config` in the convert step", weight_config=fq, step="convert")
    refused("Int4WeightFakeQuantizeConfig was passed as `base_config`. Did you mean to do the following instead?\n"
            "    qat_config = QATConfig(\n"
            "        activation_config=Int4WeightFakeQuantizeConfig(...),\n"
            "        weight_config=Int4WeightFakeQuantizeConfig(...),\n"
            '        step="prepare",\n'
            "    )", fq)


def test_infer_fake_quantize_configs():
    act, weight = _infer_fake_quantize_configs(Int4WeightOnlyConfig(group_size=64))
    assert act is None and weight == Int4WeightFakeQuantizeConfig(group_size=64, activation_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="Packing format must be one of"):
        _infer_fake_quantize_configs(Int4WeightOnlyConfig(int4_packing_format="tile_packed_to_4d"))
    base = Float8DynamicActivationFloat8WeightConfig(granularity=PerRow(), activation_value_lb=1e-12, activation_value_ub=7.0)
    act, weight = _infer_fake_quantize_configs(base)
    assert act == Float8FakeQuantizeConfig(torch.float8_e4m3fn, PerRow(), 1e-12, 7.0)
    assert weight == Float8FakeQuantizeConfig(torch.float8_e4m3fn, PerRow(), None, None)
    with pytest.raises(NotImplementedError, match=r"only PerRow\(\)"):
        _infer_fake_quantize_configs(Float8DynamicActivationFloat8WeightConfig())  # PerTensor, the base config's default
    for other in (Float8DynamicActivationInt4WeightConfig(), Int8WeightOnlyConfig()):
        with pytest.raises(ValueError, match="Unexpected base config: "):
            _infer_fake_quantize_configs(other)


def test_from_config_picks_the_quantizer():
    assert isinstance(FakeQuantizerBase.from_config(Int4WeightFakeQuantizeConfig(32)), Int4WeightFakeQuantizer)
    assert isinstance(FakeQuantizerBase.from_config(Float8FakeQuantizeConfig()), Float8FakeQuantizer)
    with pytest.raises(ValueError, match="Unknown config type"):
        FakeQuantizerBase.from_config(Int4WeightOnlyConfig())


# ---- module swaps -----------------------------------------------------------------------------------------------------------------------
def _model():
    return nn.Sequential(nn.Linear(64, 32, bias=True), nn.ReLU(), nn.Linear(32, 16, bias=False), nn.Embedding(4, 8)).to(torch.bfloat16)


def test_prepare_and_convert_swap_modules_on_a_cpu_model():
    model = _model()
    w0, b0, w2 = model[0].weight, model[0].bias, model[2].weight
    quantize_(model, QATConfig(Int4WeightOnlyConfig(group_size=32), step="prepare"))
    assert type(model[0]) is FakeQuantizedLinear and type(model[2]) is FakeQuantizedLinear and type(model[3]) is nn.Embedding
    assert model[0].weight is w0 and model[0].bias is b0 and model[2].weight is w2 and model[2].bias is None
    assert model[0].activation_fake_quantizer is None
    assert model[0].weight_fake_quantizer.config == Int4WeightFakeQuantizeConfig(32, torch.bfloat16)
    quantize_(model, QATConfig(step="convert"))  # no base config: just the swap back
    assert type(model[0]) is nn.Linear and type(model[2]) is nn.Linear
    assert model[0].weight is w0 and model[0].bias is b0 and model[2].weight is w2


def test_prepare_with_explicit_configs_and_filter_fn():
    model = _model()
    act, weight = Float8FakeQuantizeConfig(hp_value_lb=1e-12), Float8FakeQuantizeConfig()
    quantize_(model, QATConfig(activation_config=act, weight_config=weight, step="prepare"), filter_fn=lambda m, fqn: fqn == "2")
    assert type(model[0]) is nn.Linear and type(model[2]) is FakeQuantizedLinear
    assert model[2].activation_fake_quantizer.config is act and model[2].weight_fake_quantizer.config is weight
    with pytest.raises(ValueError, match="does not have QAT support"):
        quantize_(model, QATConfig(weight_config=weight, step="prepare"), filter_fn=lambda m, fqn: isinstance(m, nn.Embedding))
    # other modules pass through the convert step
    quantize_(model, QATConfig(step="convert"), filter_fn=lambda m, fqn: not isinstance(m, nn.Sequential))
    assert type(model[2]) is nn.Linear and type(model[3]) is nn.Embedding


def test_from_linear_and_to_linear_share_the_parameters():
    lin = nn.Linear(32, 16, bias=True).to(torch.bfloat16)
    fq = FakeQuantizedLinear.from_linear(lin, None, Int4WeightFakeQuantizeConfig(32))
    assert fq.weight is lin.weight and fq.bias is lin.bias and (fq.in_features, fq.out_features) == (32, 16)
    back = fq.to_linear()
    assert type(back) is nn.Linear and back.weight is lin.weight and back.bias is lin.bias
    plain = FakeQuantizedLinear(32, 16)
    assert plain.bias is None and plain.activation_fake_quantizer is None and plain.weight_fake_quantizer is None
    x = torch.randn(3, 32)
    assert torch.equal(plain(x), nn.functional.linear(x, plain.weight))  # no quantizer: a plain linear, on any device


def test_disabled_quantizers_return_their_input_and_enabled_ones_need_a_gpu():
    x = torch.randn(4, 32).to(torch.bfloat16)
    for fq in (Int4WeightFakeQuantizer(Int4WeightFakeQuantizeConfig(32)), Float8FakeQuantizer(Float8FakeQuantizeConfig())):
        assert fq.enabled is True
        with pytest.raises(RuntimeError, match="expected all tensors on the GPU.*no CPU fallback"):
            fq(x)
        fq.enabled = False
        assert fq(x) is x


def test_ops_refuse_on_the_host_before_they_ask_for_a_gpu():
    x = torch.randn(4, 128).to(torch.bfloat16)
    for fn in (ops.qat_int4_fake_quantize, ops.qat_fp8_fake_quantize_rowwise):
        with pytest.raises(RuntimeError, match="must be bfloat16, got torch.float32"):
            fn(x.float())
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)
    with pytest.raises(RuntimeError, match="grad_out must be bfloat16, got torch.float16"):
        ops.qat_int4_fake_quantize_bwd(x, x.half(), 32)
    with pytest.raises(ValueError, match="group_size must be one of 32, 64, 128, 256, got 16"):
        ops.qat_int4_fake_quantize(x, 16)
    with pytest.raises(ValueError, match="K=64 must be a multiple of group_size=128"):
        ops.qat_int4_fake_quantize(x[:, :64], 128)
    with pytest.raises(RuntimeError, match="w must be 2-D"):
        ops.qat_int4_fake_quantize(x.reshape(2, 2, 128), 32)
    with pytest.raises(ValueError, match="C=24 must be a multiple of 16"):
        ops.qat_fp8_fake_quantize_rowwise(x[:, :24])
    with pytest.raises(ValueError, match="hp_value_lb=2.0 must not exceed hp_value_ub=1.0"):
        ops.qat_fp8_fake_quantize_rowwise(x, 2.0, 1.0)
    with pytest.raises(RuntimeError, match="grad_out has shape"):
        ops.qat_fp8_fake_quantize_rowwise_bwd(x, x[:2])


def test_names_are_exported():
    for name in ("qat_int4_fake_quantize", "qat_int4_fake_quantize_bwd", "qat_fp8_fake_quantize_rowwise", "qat_fp8_fake_quantize_rowwise_bwd"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    assert set(qat.__all__) == {"QATConfig", "QATStep", "FakeQuantizeConfigBase", "Float8FakeQuantizeConfig", "Int4WeightFakeQuantizeConfig",
                                "FakeQuantizerBase", "Float8FakeQuantizer", "Int4WeightFakeQuantizer", "FakeQuantizedLinear"}
    for name in qat.__all__:
        assert hasattr(qat, name)


# ---- the C entries' host validation (nothing is launched) -------------------------------------------------------------------------------
def test_c_entries_validate_on_the_host():
    lib = _lib.lib()
    one, inv, null, ok = ctypes.c_void_p(16), _lib.AO_ERR_INVALID_ARGUMENT, _lib.AO_ERR_NULL_POINTER, _lib.AO_OK
    inf = math.inf
    for n in ("ao_qat_int4_fake_quantize", "ao_qat_int4_fake_quantize_bwd", "ao_qat_fp8_fake_quantize_rowwise",
              "ao_qat_fp8_fake_quantize_rowwise_bwd"):
        assert n in _lib.declared_symbols() and n in _lib._SIGNATURES
    assert lib.ao_abi_version() == 2
    int4 = ((lib.ao_qat_int4_fake_quantize, (one, one)), (lib.ao_qat_int4_fake_quantize_bwd, (one, one, one)))
    for fn, ptrs in int4:
        assert fn(*ptrs, 4, 96, 48, None) == inv and "group_size must be one of 32, 64, 128, 256, got 48" in _lib.last_error()
        assert fn(*ptrs, 4, 96, 64, None) == inv and "K=96 must be a multiple of group_size=64" in _lib.last_error()
        assert fn(*ptrs, -1, 64, 64, None) == inv and "bad shape" in _lib.last_error()
        assert fn(*ptrs, 1 << 40, 1 << 30, 32, None) == inv and "too large" in _lib.last_error()
        assert fn(*ptrs, 0, 96, 32, None) == ok  # K % 128 is not asked for; N == 0 launches nothing
        assert fn(*((None,) * len(ptrs)), 0, 96, 32, None) == ok
        for i in range(len(ptrs)):
            args = list(ptrs)
            args[i] = None
            assert fn(*args, 4, 96, 32, None) == null and "null pointer" in _lib.last_error()
            args[i] = ctypes.c_void_p(24)
            assert fn(*args, 4, 96, 32, None) == inv and "16-byte aligned" in _lib.last_error()
    fp8 = ((lib.ao_qat_fp8_fake_quantize_rowwise, (one, one)), (lib.ao_qat_fp8_fake_quantize_rowwise_bwd, (one, one, one)))
    for fn, ptrs in fp8:
        assert fn(*ptrs, 4, 24, -inf, inf, None) == inv and "C=24 must be a multiple of 16" in _lib.last_error()
        assert fn(*ptrs, -1, 16, -inf, inf, None) == inv and "bad shape" in _lib.last_error()
        assert fn(*ptrs, 1 << 31, 16, -inf, inf, None) == inv and "too large" in _lib.last_error()
        assert fn(*ptrs, 4, 16, 2.0, 1.0, None) == inv and "must not exceed" in _lib.last_error()
        assert fn(*ptrs, 0, 16, -inf, inf, None) == ok
        for i in range(len(ptrs)):
            args = list(ptrs)
            args[i] = None
            assert fn(*args, 4, 16, 1e-12, inf, None) == null and "null pointer" in _lib.last_error()
            args[i] = ctypes.c_void_p(8)
            assert fn(*args, 4, 16, 1e-12, inf, None) == inv and "16-byte aligned" in _lib.last_error()
