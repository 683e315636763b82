"""CPU: float8 rowwise training of the MoE grouped GEMM -- the numpy restatement of its casts and GEMMs against the fixture written from
the reference (tests/golden/fp8_grouped_training.npz); every refusal with its reason and no GPU; the config mirror; quantize_ and the
weight wrapper; the ops' registrations; the C entry points' argument checks (no kernel is launched in this file)."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
from torch import nn

import fp8_grouped_training_ref as R
from ao_amd import _lib, ops, torch_ops  # noqa: F401
from ao_amd.prototype import fp8_grouped_training as FG
from ao_amd.prototype import mx_training
from ao_amd.prototype.fp8_grouped_training import (Float8TrainingOpConfig, Float8TrainingRecipe, Float8TrainingWeightWrapperTensor,
                                                   _to_fp8_rowwise_then_scaled_grouped_mm)
from ao_amd.quantization.quant_api import quantize_

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MAKER = _load("make_golden_fp8_grouped_training")


@functools.lru_cache(maxsize=None)
def fixture():
    return MAKER.load()


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same_scale(s, want):
    np.testing.assert_array_equal(_u32(s).reshape(want.shape), _u32(want))


# ---- the restatement against the recording ---------------------------------------------------------------------------------------------
def test_the_restatement_reproduces_every_recorded_cast():
    G = fixture()
    w_t = np.ascontiguousarray(G["w"].transpose(0, 2, 1))  # B_t [E, K, N]
    for key, t in (("a_r", G["a"]), ("go_r", G["go"])):
        q, s, _ = R.rowwise(t)
        np.testing.assert_array_equal(q, G[key + "_q"])
        _same_scale(s, G[key + "_s"])
    # B_t along K (dim -2): the rowwise cast of the [E N, K] weight, transposed back
    q, s, _ = R.rowwise(G["w"].reshape(-1, MAKER.K))
    np.testing.assert_array_equal(q.reshape(MAKER.E, MAKER.N, MAKER.K).transpose(0, 2, 1), G["bt_c_q"])
    _same_scale(s, G["bt_c_s"])
    # the 3-D transposing cast: W [E, N, K] along N, codes stored [E][K][N]
    q, s, _ = R.colwise_3d(G["w"])
    np.testing.assert_array_equal(q.transpose(0, 2, 1), G["w3_q"])
    _same_scale(s, G["w3_s"])
    assert G["w3_q"].shape == w_t.shape
    for key, t in (("go_j", G["go"]), ("a_j", G["a"])):
        q, s, inv = R.group_colwise(t, G["offs"])
        np.testing.assert_array_equal(q, G[key + "_q"])
        _same_scale(s, G[key + "_s"])  # [E, C] group-major is the reference's [E * C] vector
        np.testing.assert_array_equal(_u32(inv), _u32(1.0 / torch.from_numpy(s.copy())))
    for key in G:
        if key.endswith("_s"):
            assert np.all((_u32(G[key]) & 0x7FFFFF) == 0), key  # every recorded scale is a power of two


def test_the_restatement_reproduces_every_recorded_output():
    G = fixture()
    offs = G["offs"]
    out = R.grouped_mm(G["a_r_q"], G["a_r_s"], G["bt_c_q"].transpose(0, 2, 1), G["bt_c_s"].reshape(MAKER.E, MAKER.N), offs)
    grad_a = R.grouped_mm(G["go_r_q"], G["go_r_s"], G["w3_q"], G["w3_s"].reshape(MAKER.E, MAKER.K), offs)
    grad_w = R.wgrad(G["go_j_q"], G["go_j_s"].reshape(MAKER.E, MAKER.N), G["a_j_q"], G["a_j_s"].reshape(MAKER.E, MAKER.K), offs)
    for name, y in (("out", out), ("grad_a", grad_a), ("grad_w", grad_w)):
        got, want = R.to_bf16_bits(y).astype(np.int32), G[name].astype(np.int32)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1, name  # (the same sign everywhere a bf16 ulp is one step of the bits)
        np.testing.assert_array_equal(got, want)    # the float64 sums are the recorder's own: exact


def test_the_restatements_rules_for_empty_groups_and_tail_rows():
    G = fixture()
    x = G["a"][:64, :16]
    q, s, inv = R.group_colwise(x, [16, 16, 48])
    assert np.all(s[1] == np.float32(2.0 ** 48)) and np.all(inv[1] == np.float32(2.0 ** -48))  # 448 / 1e-12 = 4.48e14, rounded down
    assert not q[48:].any() and q[:48].any()
    q0, s0, _ = R.group_colwise(x, [16, 16, 48], pow2=False)
    assert np.all(s0[1] == np.float32(448.0 / 1e-12))
    np.testing.assert_array_equal(q[:16], R.T.cast(x[:16], 0, True)[0])
    assert not R.wgrad(q, s, q, s, [16, 16, 48])[1].any()


# ---- refusals, each before any launch ------------------------------------------------------------------------------------------------------
def _operands(m=32, k=128, n=128, e=2):
    a = torch.zeros(m, k, dtype=torch.bfloat16)
    b_t = torch.zeros(e, n, k, dtype=torch.bfloat16).transpose(-2, -1)
    offs = torch.tensor([16, 32][:e], dtype=torch.int32)
    return a, b_t, offs


@pytest.mark.parametrize("change,message", [
    (lambda a, b, o: (a[None], b, o), "A must be 2D"),
    (lambda a, b, o: (a, b[0], o), "B must be 3D"),
    (lambda a, b, o: (a.float(), b, o), "A must be bfloat16"),
    (lambda a, b, o: (a, b.to(torch.float16), o), "B must be bfloat16"),
    (lambda a, b, o: (a, b, o.long()), "offs must be an int32 tensor"),
    (lambda a, b, o: (a, b, None), "offs must be an int32 tensor"),
    (lambda a, b, o: (a, b, o[:1]), "one end per expert"),
    (lambda a, b, o: (a[:, :64], b, o), "not compatible"),
    (lambda a, b, o: (torch.zeros(128, 32, dtype=torch.bfloat16).t(), b, o), "A must be row-major"),
    (lambda a, b, o: (a, b.contiguous(), o), "B must be column-major"),
    (lambda a, b, o: (torch.zeros(32, 64, dtype=torch.bfloat16), torch.zeros(2, 128, 64, dtype=torch.bfloat16).transpose(-2, -1), o),
     "K and N must be multiples of 128.*K=64 N=128"),
    (lambda a, b, o: (a, torch.zeros(2, 64, 128, dtype=torch.bfloat16).transpose(-2, -1), o), "K and N must be multiples of 128.*K=128 N=64"),
], ids=["a-3d", "b-2d", "a-f32", "b-f16", "offs-i64", "offs-none", "offs-len", "shapes", "a-colmajor", "b-rowmajor", "k-64", "n-64"])
def test_operands_that_the_function_does_not_take_are_refused_on_the_cpu(change, message):
    a, b_t, offs = change(*_operands())
    with pytest.raises(AssertionError, match=message):
        _to_fp8_rowwise_then_scaled_grouped_mm(a, b_t, offs)


def test_dtypes_and_token_counts_are_refused_and_the_gpu_requirement_comes_last():
    a, b_t, offs = _operands()
    with pytest.raises(AssertionError, match="float8_dtype must be torch.float8_e4m3fn"):
        _to_fp8_rowwise_then_scaled_grouped_mm(a, b_t, offs, float8_dtype=torch.float8_e5m2)
    with pytest.raises(AssertionError, match="Only bfloat16 out_dtype"):
        _to_fp8_rowwise_then_scaled_grouped_mm(a, b_t, offs, out_dtype=torch.float32)
    a24 = torch.zeros(24, 128, dtype=torch.bfloat16)
    with pytest.raises(AssertionError, match="M=24 tokens must be a multiple of 16.*pad_token_groups_for_grouped_mm=True"):
        _to_fp8_rowwise_then_scaled_grouped_mm(a24, b_t, offs, pad_token_groups_for_grouped_mm=False)
    for args, kw in (((a24, b_t, offs), {}), ((a, b_t, offs), dict(pad_token_groups_for_grouped_mm=False))):  # accepted: only the GPU is missing
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _to_fp8_rowwise_then_scaled_grouped_mm(*args, **kw)


# ---- the config ------------------------------------------------------------------------------------------------------------------------------
def test_the_config_mirrors_the_references():
    c = Float8TrainingOpConfig()
    assert (c.float8_dtype, c.out_dtype, c.pad_token_groups_for_grouped_mm, c.float8_linear_recipe) == (
        torch.float8_e4m3fn, torch.bfloat16, False, "rowwise")
    assert Float8TrainingOpConfig.from_recipe(Float8TrainingRecipe.FP8_ROWWISE) == c
    assert hash(Float8TrainingOpConfig.from_recipe(Float8TrainingRecipe.FP8_ROWWISE)) == hash(c)
    assert Float8TrainingRecipe("fp8_rowwise") is Float8TrainingRecipe.FP8_ROWWISE and len(Float8TrainingRecipe) == 1
    for other in (Float8TrainingOpConfig(pad_token_groups_for_grouped_mm=True), Float8TrainingOpConfig(out_dtype=torch.float32),
                  Float8TrainingOpConfig(float8_linear_recipe="rowwise_with_gw_hp"), Float8TrainingOpConfig(float8_dtype=torch.float8_e5m2)):
        assert other != c and len({other, c}) == 2
    assert c != mx_training.MXFP8TrainingOpConfig() and c != "rowwise"
    with pytest.raises(ValueError, match="Unsupported FP8 recipe"):
        Float8TrainingOpConfig.from_recipe(mx_training.MXFP8TrainingRecipe.MXFP8_RCEIL)
    with pytest.raises(AssertionError, match="not in valid names"):
        Float8TrainingOpConfig(float8_linear_recipe="blockwise")
    assert c._float8_linear_config.round_scales_to_power_of_2 and c._linear_mm_config.output.use_fast_accum
    assert set(FG.__all__) >= {"_to_fp8_rowwise_then_scaled_grouped_mm", "_Float8GroupedMM", "Float8TrainingRecipe", "Float8TrainingOpConfig",
                               "Float8TrainingWeightWrapperTensor"}
    import ao_amd.prototype as P
    assert all(hasattr(P, n) and n in P.__all__ for n in FG.__all__)


# ---- quantize_ and the wrapper ---------------------------------------------------------------------------------------------------------------
class Experts(nn.Module):
    def __init__(self):
        super().__init__()
        self.w1 = nn.Parameter(torch.randn(2, 128, 128, dtype=torch.bfloat16))
        self.w2 = nn.Parameter(torch.randn(2, 128, 128, dtype=torch.bfloat16), requires_grad=False)


class Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.experts = Experts()
        self.router = nn.Linear(128, 2, bias=False).to(torch.bfloat16)
        self.proj = nn.Linear(128, 128).to(torch.bfloat16)


def test_quantize_wraps_exactly_the_filtered_parameters_and_keeps_requires_grad():
    cfg = Float8TrainingOpConfig()
    model = Toy()
    quantize_(model, cfg, filter_fn=lambda mod, fqn: fqn in ("experts", "proj"))
    kinds = {n: type(p.data) for n, p in model.named_parameters()}
    W = Float8TrainingWeightWrapperTensor
    assert kinds == {"experts.w1": W, "experts.w2": W, "router.weight": torch.Tensor, "proj.weight": W, "proj.bias": W}
    assert model.experts.w1.requires_grad and not model.experts.w2.requires_grad and isinstance(model.experts.w1, nn.Parameter)
    assert model.experts.w1.data.config is cfg
    before = model.experts.w1
    quantize_(model, cfg, filter_fn=lambda mod, fqn: fqn == "experts")  # a wrapped parameter is left as it is
    assert model.experts.w1 is before
    # the MXFP8 config still gets its own wrapper, an unknown config is refused
    m2 = mx_training._swap_params(Experts(), config=mx_training.MXFP8TrainingOpConfig())
    assert type(m2.w1.data) is mx_training.MXFP8TrainingWeightWrapperTensor
    with pytest.raises(AssertionError, match="Unsupported config type"):
        mx_training._swap_params(Experts(), config=object())


def test_the_wrapper_is_a_plain_tensor_for_other_ops_and_routes_the_gemms():
    cfg = Float8TrainingOpConfig()
    w = torch.randn(2, 128, 128, dtype=torch.bfloat16)
    t = Float8TrainingWeightWrapperTensor(w.clone(), cfg)
    assert type(t + 1) is torch.Tensor and torch.equal(t + 1, w + 1)
    assert type(t.sum()) is torch.Tensor and type(t.detach()) is Float8TrainingWeightWrapperTensor
    tt = t.transpose(-2, -1)
    assert type(tt) is Float8TrainingWeightWrapperTensor and tt.config is cfg and tt.stride() == (128 * 128, 1, 128)
    assert type(t[0]) is torch.Tensor or type(t[0]) is Float8TrainingWeightWrapperTensor
    assert "Float8TrainingWeightWrapperTensor" in repr(t)
    names, ctx = t.__tensor_flatten__()
    assert names == ["_data"] and Float8TrainingWeightWrapperTensor.__tensor_unflatten__({"_data": w}, ctx, None, None).config is cfg
    other = Float8TrainingWeightWrapperTensor(w.clone(), Float8TrainingOpConfig(pad_token_groups_for_grouped_mm=True))
    with pytest.raises(AssertionError, match="must have the same config"):
        t + other
    x = torch.zeros(32, 128, dtype=torch.bfloat16)
    offs = torch.tensor([16, 32], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the float8 Function took the call and got as far as its first launch
        torch._grouped_mm(x, tt, offs=offs)
    with pytest.raises(AssertionError, match="M=24 tokens must be a multiple of 16"):
        torch._grouped_mm(x[:24], tt, offs=offs)
    lin = Float8TrainingWeightWrapperTensor(torch.zeros(64, 128, dtype=torch.bfloat16), cfg)
    for call in (lambda: torch.nn.functional.linear(x, lin), lambda: torch.mm(x, lin.t()), lambda: torch.matmul(x, lin.t()),
                 lambda: torch.addmm(torch.zeros(64, dtype=torch.bfloat16), x, lin.t())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(AssertionError, match="K and N must be multiples of 16"):
        torch.nn.functional.linear(x[:, :24], Float8TrainingWeightWrapperTensor(torch.zeros(64, 24, dtype=torch.bfloat16), cfg))
    ten = Float8TrainingWeightWrapperTensor(torch.zeros(64, 128, dtype=torch.bfloat16), Float8TrainingOpConfig(float8_linear_recipe="tensorwise"))
    with pytest.raises(ValueError, match="float8_e5m2"):  # check_config's refusal, as for Float8Linear
        torch.nn.functional.linear(x, ten)


# ---- the ops ---------------------------------------------------------------------------------------------------------------------------------
def test_the_ops_exist_refuse_the_cpu_and_are_registered_with_fakes():
    names = ("fp8_train_quantize_group_colwise_t", "fp8_train_quantize_colwise_t_3d", "fp8_grouped_mm_wgrad")
    for n in names:
        assert n in ops.__all__ and callable(getattr(ops, n)) and hasattr(torch.ops.ao_mi355, n)
    x = torch.zeros(32, 48, dtype=torch.bfloat16)
    offs = torch.tensor([16, 32], dtype=torch.int32)
    q = torch.zeros(48, 32, dtype=torch.float8_e4m3fn)
    inv = torch.zeros(2, 48)
    for call in (lambda: ops.fp8_train_quantize_group_colwise_t(x, offs), lambda: ops.fp8_train_quantize_colwise_t_3d(x[None]),
                 lambda: ops.fp8_grouped_mm_wgrad(q, inv, q, inv, offs, 48, 48)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        fx = torch.empty(32, 48, dtype=torch.bfloat16, device="cuda")
        fo = torch.empty(2, dtype=torch.int32, device="cuda")
        qt, s, i = torch.ops.ao_mi355.fp8_train_quantize_group_colwise_t(fx, fo, True)
        assert (tuple(qt.shape), qt.dtype, tuple(s.shape), tuple(i.shape), s.dtype) == ((48, 32), torch.float8_e4m3fn, (2, 48), (2, 48), torch.float32)
        qt3, s3, i3 = torch.ops.ao_mi355.fp8_train_quantize_colwise_t_3d(fx.view(2, 16, 48), True)
        assert (tuple(qt3.shape), qt3.dtype, tuple(s3.shape), tuple(i3.shape)) == ((2, 48, 16), torch.float8_e4m3fn, (2, 48), (2, 48))
        out = torch.ops.ao_mi355.fp8_grouped_mm_wgrad(qt, i, qt, i, fo, 48, 48)
        assert (tuple(out.shape), out.dtype) == ((2, 48, 48), torch.bfloat16)
        assert tuple(torch.ops.ao_mi355.fp8_grouped_mm_wgrad(qt, i[:1], qt, i[:1], None, 48, 48).shape) == (1, 48, 48)


# ---- the C entry points ----------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_and_exported():
    names = _lib.declared_symbols()
    for n in ("ao_fp8_train_quantize_group_colwise_t", "ao_fp8_train_quantize_colwise_t_3d", "ao_fp8_grouped_mm_wgrad"):
        assert n in names and n in _lib._SIGNATURES and hasattr(_lib.lib(), n)


def test_the_entry_points_check_their_arguments_on_the_host():
    lib = _lib.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first, and an empty matrix launches nothing
    inv, ok, null = _lib.AO_ERR_INVALID_ARGUMENT, _lib.AO_OK, _lib.AO_ERR_NULL_POINTER
    jag = lambda r, c, e=2, x=one, offs=one: lib.ao_fp8_train_quantize_group_colwise_t(x, offs, one, one, one, 1, r, c, e, None)  # noqa: E731
    c3d = lambda e, r, c, w=one: lib.ao_fp8_train_quantize_colwise_t_3d(w, one, one, one, 1, e, r, c, None)  # noqa: E731
    wg = lambda m, n, k, e=2, g=one, offs=one, out=one: lib.ao_fp8_grouped_mm_wgrad(g, one, one, one, offs, out, m, n, k, e, None)  # noqa: E731
    assert jag(24, 32) == inv and "R=24 must be a multiple of 16" in _lib.last_error()
    assert jag(32, 24) == inv and "C=24 must be a multiple of 16" in _lib.last_error()
    assert jag(32, 32, e=0) == inv and jag(32, 32, e=65536) == inv and "E=65536" in _lib.last_error()
    assert jag(65535 * 128 + 16, 32) == inv and "too large" in _lib.last_error()
    assert jag(0, 32) == ok and jag(32, 0) == ok and jag(0, 24) == inv
    assert jag(32, 32, x=None) == null and jag(32, 32, offs=None) == null
    assert c3d(2, 24, 32) == inv and "R=24" in _lib.last_error()
    assert c3d(2, 32, 24) == inv and "C=24" in _lib.last_error()
    assert c3d(-1, 32, 32) == inv and c3d(65535, 256, 32) == inv and "too large" in _lib.last_error()
    assert c3d(0, 32, 32) == ok and c3d(2, 0, 32) == ok and c3d(2, 32, 0) == ok
    assert c3d(2, 32, 32, w=None) == null
    assert wg(24, 32, 32) == inv and "M_total=24 must be a multiple of 16" in _lib.last_error()
    assert wg(32, 24, 32) == inv and "N=24" in _lib.last_error()
    assert wg(32, 32, 24) == inv and "K=24" in _lib.last_error()
    assert wg(32, 32, 32, e=0) == inv and wg(32, 32, 32, e=65536) == inv
    assert wg(32, 32, 32, e=2, offs=None) == inv and "one group" in _lib.last_error()
    assert wg(1 << 20, 4096, 32) == inv and "below 2^31" in _lib.last_error()
    assert wg(32, 32, 32, out=None) == null and wg(32, 32, 32, g=None) == null
    with pytest.raises(ValueError):
        _lib.check(jag(24, 32))
