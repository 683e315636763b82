"""CPU: MXFP8 dense-linear training at the host -- the two new entries' declarations, exports and argument checks, the fake kernels of
their dispatcher ops, MXFP8TrainingOpConfig and its recipes, the refusals of _to_mxfp8_then_scaled_mm, the weight wrapper tensor and
quantize_ on CPU tensors, and the fixture written from the reference (tests/golden/mxfp8_linear_bwd.npz) against the oracle's cast.
No kernel is launched in this file."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch
from torch import nn

from ao_amd import _lib, ops
from ao_amd.prototype import mx, mx_training as T
from ao_amd.quantization import KernelPreference, quantize_
from oracle import mx_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROWCOL, WGRAD = "ao_mxfp8_quantize_rowcol", "ao_mxfp8_mm_wgrad"
RCEIL, FLOOR = mx.ScaleCalculationMode.RCEIL, mx.ScaleCalculationMode.FLOOR


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_mxfp8_linear_bwd", os.path.join(HERE, "golden", "make_golden_mxfp8_linear_bwd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bf16(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_signed():
    lib = _lib.lib()
    for name, nargs in ((ROWCOL, 9), (WGRAD, 9)):
        assert hasattr(lib, name) and name in _lib.declared_symbols() and name in _lib._SIGNATURES
        assert len(_lib._SIGNATURES[name]) == nargs
    assert "mxfp8_quantize_rowcol" in ops.__all__ and "mxfp8_mm_wgrad" in ops.__all__
    assert list(inspect.signature(ops.mxfp8_quantize_rowcol).parameters) == ["x", "scaling_mode"]
    assert list(inspect.signature(ops.mxfp8_mm_wgrad).parameters) == ["g_t", "g_scale", "x_t", "x_scale", "N", "K"]


def _scratch():
    buf = ctypes.create_string_buffer(4096)
    return buf, (ctypes.addressof(buf) + 15) & ~15


@pytest.mark.parametrize("shape,mode,reason", [
    ((48, 64), 1, "R=48 must be a multiple of 32"),
    ((64, 48), 1, "K=48 must be a multiple of 32"),
    ((64, 0), 1, "bad shape"),
    ((-32, 64), 1, "bad shape"),
    ((64, 64), 2, "scaling_mode must be AO_MX_SCALE_FLOOR or AO_MX_SCALE_RCEIL"),
    ((65536 * 128, 32), 1, "too large for one launch"),
])
def test_the_cast_rejects_the_shape_with_a_reason(shape, mode, reason):
    lib = _lib.lib()
    _buf, p = _scratch()
    assert getattr(lib, ROWCOL)(p, p, p, p, p, *shape, mode, None) == _lib.AO_ERR_INVALID_ARGUMENT
    msg = lib.ao_last_error().decode()
    assert ROWCOL in msg and reason in msg, msg


def test_the_cast_rejects_null_pointers_and_takes_no_rows():
    lib = _lib.lib()
    _buf, p = _scratch()
    fn = getattr(lib, ROWCOL)
    for i in range(5):  # x, q_row, s_row, q_col_t, s_col
        args = [p] * 5
        args[i] = None
        assert fn(*args, 64, 64, 1, None) == _lib.AO_ERR_NULL_POINTER, i
    assert fn(None, None, None, None, None, 0, 64, 1, None) == _lib.AO_OK  # R == 0: nothing to launch


@pytest.mark.parametrize("shape,reason", [
    ((48, 128, 128), "M_total=48 must be a multiple of 32"),
    ((64, 24, 128), "N=24 must be a multiple of 16"),
    ((64, 128, 40), "K=40 must be a multiple of 16"),
    ((64, 0, 128), "bad shape"),
    ((1 << 20, 1 << 11, 128), "below 2^31"),
    ((1 << 20, 128, 1 << 11), "below 2^31"),
])
def test_the_dense_wgrad_has_the_grouped_entrys_checks(shape, reason):
    lib = _lib.lib()
    _buf, p = _scratch()
    assert getattr(lib, WGRAD)(p, p, p, p, p, *shape, None) == _lib.AO_ERR_INVALID_ARGUMENT
    msg = lib.ao_last_error().decode()
    assert WGRAD in msg and reason in msg, msg
    fn = getattr(lib, WGRAD)
    for i in range(5):  # g_t, g_scale, x_t, x_scale, out
        args = [p] * 5
        args[i] = None
        assert fn(*args, 64, 128, 128, None) == _lib.AO_ERR_NULL_POINTER, i
        assert WGRAD + ": null pointer" in lib.ao_last_error().decode()
    assert fn(p + 8, p, p, p, p, 64, 128, 128, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert "16-byte aligned" in lib.ao_last_error().decode()


def test_ops_check_before_any_launch():
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    with pytest.raises(RuntimeError, match="mxfp8_mm_wgrad: .*no CPU fallback"):
        ops.mxfp8_mm_wgrad(z(128, 64), z(2, 128), z(128, 64), z(2, 128), 128, 128)
    with pytest.raises(RuntimeError, match="mxfp8_quantize_rowcol: .*no CPU fallback"):
        ops.mxfp8_quantize_rowcol(torch.zeros(32, 32, dtype=torch.bfloat16))


def test_fake_kernels_give_shapes_strides_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import ao_amd.torch_ops  # noqa: F401

    with FakeTensorMode():
        q, s, q_t, s_t = torch.ops.ao_mi355.mxfp8_quantize_rowcol(torch.empty(64, 96, dtype=torch.bfloat16), "rceil")
        g_t, x_t = torch.empty(64, 128, dtype=torch.float8_e4m3fn).t(), torch.empty(256, 128, dtype=torch.float8_e4m3fn).t()
        gs, xs = torch.empty(4, 64, dtype=torch.float8_e8m0fnu).t(), torch.empty(4, 256, dtype=torch.float8_e8m0fnu).t()
        y = torch.ops.ao_mi355.mxfp8_mm_wgrad(g_t, gs, x_t, xs, 64, 256)
    assert tuple(q.shape) == (64, 96) and q.stride() == (96, 1) and q.dtype == torch.float8_e4m3fn
    assert tuple(s.shape) == (64, 3) and s.stride() == (3, 1) and s.dtype == torch.float8_e8m0fnu
    # the views mxfp8_quantize_colwise returns: {R, C} with strides {1, R}; {C, R / 32} with strides {1, C}
    assert tuple(q_t.shape) == (64, 96) and q_t.stride() == (1, 64) and q_t.dtype == torch.float8_e4m3fn
    assert tuple(s_t.shape) == (96, 2) and s_t.stride() == (1, 96) and s_t.dtype == torch.float8_e8m0fnu
    assert tuple(y.shape) == (64, 256) and y.stride() == (256, 1) and y.dtype == torch.bfloat16


# ---- the config ----------------------------------------------------------------------------------------------------------------------------
def test_the_config_compares_hashes_and_builds_from_recipes():
    C, R = T.MXFP8TrainingOpConfig, T.MXFP8TrainingRecipe
    d = C()
    assert (d.kernel_preference, d.out_dtype, d.wgrad_with_hp, d.scale_calculation_mode, d.pad_token_groups_for_grouped_mm) == (
        KernelPreference.AUTO, torch.bfloat16, False, RCEIL, False)
    assert [f for f in C.__dataclass_fields__] == ["kernel_preference", "out_dtype", "wgrad_with_hp", "scale_calculation_mode",
                                                   "pad_token_groups_for_grouped_mm"]
    assert C() == C() and hash(C()) == hash(C()) and len({C(), C(), C(wgrad_with_hp=True)}) == 2
    for other in (C(wgrad_with_hp=True), C(scale_calculation_mode=FLOOR), C(kernel_preference=KernelPreference.EMULATED),
                  C(pad_token_groups_for_grouped_mm=True), C(out_dtype=torch.float32)):
        assert other != d
    assert d != object() and d.__eq__(3) is NotImplemented
    assert [r.value for r in R] == ["mxfp8_rceil", "mxfp8_rceil_wgrad_with_hp", "mxfp8_emulated_rceil"]
    assert C.from_recipe(R.MXFP8_RCEIL) == d
    assert C.from_recipe(R.MXFP8_RCEIL_WGRAD_WITH_HP) == C(wgrad_with_hp=True)
    assert C.from_recipe(R.MXFP8_EMULATED_RCEIL) == C(kernel_preference=KernelPreference.EMULATED)
    with pytest.raises(ValueError, match="Unsupported MXFP8 recipe"):
        C.from_recipe("mxfp8_floor")


# ---- the Python entry ------------------------------------------------------------------------------------------------------------------------
def test_the_entries_have_the_references_names_order_and_defaults():
    assert list(inspect.signature(T._to_mxfp8_then_scaled_mm).parameters) == [
        "input_hp", "weight_hp", "kernel_preference", "scale_calculation_mode", "wgrad_with_hp"]
    assert inspect.signature(T._to_mxfp8_then_scaled_mm).parameters["wgrad_with_hp"].default is False
    assert list(inspect.signature(T.mx_mm.forward).parameters) == [
        "ctx", "input_hp", "weight_hp", "in_elem_dtype", "w_elem_dtype", "grad_elem_dtype", "block_size", "kernel_preference",
        "mxfp8_dim0_cast_kernel_choice", "mxfp8_dim1_cast_kernel_choice", "scale_calculation_mode", "wgrad_with_hp"]
    assert issubclass(T.mx_mm, torch.autograd.Function) and issubclass(T.MXFP8Linear, nn.Linear)
    lin = T.MXFP8Linear(64, 32, bias=False)
    assert (lin.kernel_preference, lin.scale_calculation_mode, lin.wgrad_with_hp) == (KernelPreference.AUTO, RCEIL, False)
    import ao_amd.prototype as P

    for name in ("MXFP8Linear", "MXFP8TrainingOpConfig", "MXFP8TrainingRecipe", "MXFP8TrainingWeightWrapperTensor", "mx_mm",
                 "_to_mxfp8_then_scaled_mm"):
        assert getattr(P, name) is getattr(T, name)


def _operands(m=64, k=64, n=64, dtype=torch.bfloat16, grad=True):
    return torch.zeros(m, k, dtype=dtype, requires_grad=grad), torch.zeros(n, k, dtype=dtype, requires_grad=grad)


def test_refusals_come_with_a_reason_before_any_launch():
    f = T._to_mxfp8_then_scaled_mm
    x, w = _operands(dtype=torch.float32)
    with pytest.raises(AssertionError, match="input and weight must be bfloat16, got torch.float32 and torch.float32"):
        f(x, w, KernelPreference.AUTO, RCEIL)
    x, w = _operands()
    with pytest.raises(AssertionError, match="input and weight must be bfloat16, got torch.bfloat16 and torch.float32"):
        f(x, w.float(), KernelPreference.AUTO, RCEIL)
    x, w = _operands(k=48)
    with pytest.raises(AssertionError, match="K and N must be multiples of 32.*K=48 N=64"):
        f(x, w, KernelPreference.AUTO, RCEIL)
    x, w = _operands(n=80)
    with pytest.raises(AssertionError, match="K and N must be multiples of 32.*K=64 N=80"):
        f(x, w, KernelPreference.AUTO, RCEIL)
    x, w = _operands(m=48)
    with pytest.raises(AssertionError, match="M=48 tokens must be a multiple of 32.*wgrad_with_hp=True or freeze the weight"):
        f(x, w, KernelPreference.AUTO, RCEIL)
    with pytest.raises(AssertionError, match="M=48 tokens"):
        f(x.reshape(2, 24, 64), w, KernelPreference.EMULATED, FLOOR)
    for pref in (KernelPreference.TORCH, KernelPreference.TRITON, KernelPreference.MSLK, "cutlass"):
        with pytest.raises(AssertionError, match="KernelPreference AUTO or EMULATED"):
            f(*_operands(), pref, RCEIL)


def test_an_odd_token_count_passes_the_checks_when_no_mxfp8_wgrad_is_needed():
    """M % 32 != 0 is refused only for the MXFP8 weight gradient: with wgrad_with_hp, a frozen weight or no_grad the call reaches the
    kernels' own device check."""
    f = T._to_mxfp8_then_scaled_mm
    x, w = _operands(m=48)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, w, KernelPreference.AUTO, RCEIL, wgrad_with_hp=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, w.detach(), KernelPreference.AUTO, RCEIL)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, w, KernelPreference.EMULATED, RCEIL)


# ---- the wrapper and quantize_ -------------------------------------------------------------------------------------------------------------
W = T.MXFP8TrainingWeightWrapperTensor


def test_the_wrapper_keeps_its_class_through_the_preserved_ops_only():
    cfg = T.MXFP8TrainingOpConfig(wgrad_with_hp=True)
    data = torch.arange(24, dtype=torch.float32).reshape(4, 6).to(torch.bfloat16)
    w = W(data, cfg)
    assert isinstance(w, torch.Tensor) and w._data is data and w.config is cfg
    assert w.shape == data.shape and w.stride() == data.stride() and w.dtype == torch.bfloat16 and not w.requires_grad
    assert W(data.clone().requires_grad_(True), cfg).requires_grad
    for out, want in ((w.t(), data.t()), (w.transpose(0, 1), data.transpose(0, 1)), (w.detach(), data), (w.clone(), data),
                      (w[1:3], data[1:3]), (w.view(6, 4), data.view(6, 4)), (w.to(torch.float32), data.float())):
        assert type(out) is W and out.config is cfg and out.shape == want.shape and out.stride() == want.stride()
        assert torch.equal(out._data, want)
    assert w.detach()._data is data  # the reference's special case: the same inner tensor
    assert w.clone()._data is not data
    for out in (w + 1, w * 2, w.sum(), torch.relu(w)):  # everything else gives plain tensors
        assert type(out) is torch.Tensor
    assert torch.equal(w + 1, data + 1)
    assert "MXFP8TrainingWeightWrapperTensor(data=" in repr(w)


def test_in_place_ops_through_dispatch_mutate_the_inner_tensor():
    data = torch.ones(4, 32, dtype=torch.bfloat16)
    w = W(data, T.MXFP8TrainingOpConfig())
    w.add_(torch.full((4, 32), 2.0, dtype=torch.bfloat16), alpha=-0.5)
    assert w._data is data and torch.equal(data, torch.zeros(4, 32, dtype=torch.bfloat16))
    w.copy_(torch.full((4, 32), 3.0, dtype=torch.bfloat16))
    assert torch.equal(data, torch.full((4, 32), 3.0, dtype=torch.bfloat16))
    p = nn.Parameter(W(torch.ones(2, 32, dtype=torch.bfloat16), T.MXFP8TrainingOpConfig()))
    p.grad = torch.ones(2, 32, dtype=torch.bfloat16)
    torch.optim.SGD([p], lr=0.5).step()
    assert torch.equal(p.data._data, torch.full((2, 32), 0.5, dtype=torch.bfloat16))


def test_wrappers_of_different_configs_do_not_mix():
    a = W(torch.ones(2, 2), T.MXFP8TrainingOpConfig())
    b = W(torch.ones(2, 2), T.MXFP8TrainingOpConfig(wgrad_with_hp=True))
    with pytest.raises(AssertionError, match="must have the same config"):
        a + b


def test_flatten_and_unflatten_round_trip():
    cfg = T.MXFP8TrainingOpConfig(scale_calculation_mode=FLOOR)
    w = W(torch.randn(4, 32).to(torch.bfloat16), cfg)
    names, meta = w.__tensor_flatten__()
    assert names == ["_data"] and meta == {"config": cfg}
    back = W.__tensor_unflatten__({"_data": w._data}, meta, w.shape, w.stride())
    assert type(back) is W and back._data is w._data and back.config == cfg


class _Experts(nn.Module):
    def __init__(self):
        super().__init__()
        self.w1 = nn.Parameter(torch.zeros(2, 64, 32, dtype=torch.bfloat16))
        self.w2 = nn.Parameter(torch.zeros(2, 32, 64, dtype=torch.bfloat16), requires_grad=False)


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = nn.Linear(32, 64, bias=True, dtype=torch.bfloat16)
        self.gate = nn.Linear(32, 2, bias=False, dtype=torch.bfloat16)
        self.experts = _Experts()
        self.norm = nn.LayerNorm(32, dtype=torch.bfloat16)


def test_quantize_wraps_the_parameters_of_matching_modules_once():
    cfg = T.MXFP8TrainingOpConfig()
    m = _Block()
    quantize_(m, cfg, filter_fn=lambda mod, fqn: isinstance(mod, nn.Linear) and "gate" not in fqn)
    assert type(m.proj.weight.data) is W and type(m.proj.bias.data) is W  # weight and bias of the matching module
    assert isinstance(m.proj.weight, nn.Parameter) and m.proj.weight.requires_grad and m.proj.weight.data.config == cfg
    for p in (m.gate.weight, m.experts.w1, m.experts.w2, m.norm.weight, m.norm.bias):
        assert type(p.data) is torch.Tensor
    inner = m.proj.weight.data._data
    quantize_(m, cfg, filter_fn=lambda mod, fqn: isinstance(mod, nn.Linear) and "gate" not in fqn)
    assert type(m.proj.weight.data._data) is torch.Tensor and m.proj.weight.data._data is inner  # never twice
    # the default filter: every plain nn.Linear
    m = _Block()
    quantize_(m, cfg)
    assert type(m.proj.weight.data) is W and type(m.gate.weight.data) is W and type(m.experts.w1.data) is torch.Tensor
    # an explicit filter for the module that holds 3-D expert parameters; requires_grad is kept
    quantize_(m, cfg, filter_fn=lambda mod, fqn: fqn == "experts")
    assert type(m.experts.w1.data) is W and type(m.experts.w2.data) is W and m.experts.w1.data.ndim == 3
    assert m.experts.w1.requires_grad and not m.experts.w2.requires_grad


def test_the_handler_honours_parameter_name():
    cfg = T.MXFP8TrainingOpConfig()
    m = _Block()
    T._moe_training_transform(m.experts, cfg, parameter_name="w1")
    assert type(m.experts.w1.data) is W and type(m.experts.w2.data) is torch.Tensor
    T._swap_params(m.proj, config=cfg, target_parameter_name="weight")
    assert type(m.proj.weight.data) is W and type(m.proj.bias.data) is torch.Tensor
    p = T._swap_params(nn.Parameter(torch.zeros(2, 2), requires_grad=False), config=cfg)
    assert isinstance(p, nn.Parameter) and type(p.data) is W and not p.requires_grad
    with pytest.raises(AssertionError, match="Unsupported config type"):
        T._swap_params(m, config=object())


def test_the_wrapper_routes_matmuls_to_the_function_and_leaves_other_calls_alone():
    """On CPU tensors the routed calls end at the kernels' device check (or at a refusal of the Function's entry), other calls compute."""
    cfg = T.MXFP8TrainingOpConfig()
    w = nn.Parameter(W(torch.zeros(64, 32, dtype=torch.bfloat16), cfg))
    x = torch.zeros(32, 32, dtype=torch.bfloat16)
    for call in (lambda: torch.nn.functional.linear(x, w), lambda: torch.nn.functional.linear(x, w, torch.zeros(64, dtype=torch.bfloat16)),
                 lambda: torch.mm(x, w.t()), lambda: torch.matmul(x, w.t()), lambda: x @ w.t(),
                 lambda: torch.addmm(torch.zeros(64, dtype=torch.bfloat16), x, w.t())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(AssertionError, match="input and weight must be bfloat16"):
        torch.nn.functional.linear(x.float(), w)
    e = nn.Parameter(W(torch.zeros(2, 64, 32, dtype=torch.bfloat16), cfg))
    offs = torch.tensor([16, 32], dtype=torch.int32)
    with pytest.raises(AssertionError, match="N and K to be multiples of 128"):  # the grouped Function's own refusal: the call was routed
        torch._grouped_mm(x, e.transpose(-2, -1), offs=offs)
    assert type(torch.cat([w, w])) is torch.Tensor and torch.cat([w, w]).shape == (128, 32)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_references_casts_and_gradients():
    gen = _generator()
    G = gen.load()
    B, Tk, N, K = gen.B, gen.T, gen.N, gen.K
    M = B * Tk
    assert G["x"].shape == (B, Tk, K) and G["w"].shape == (N, K) and G["go"].shape == (B, Tk, N)
    for tag, _mode, _hp in gen.VARIANTS:
        assert G["out_" + tag].shape == (B, Tk, N) and G["gi_" + tag].shape == (B, Tk, K) and G["gw_" + tag].shape == (N, K)
        assert G["out_" + tag].dtype == G["gi_" + tag].dtype == G["gw_" + tag].dtype == np.uint16
    np.testing.assert_array_equal(G["out_rceil_hp"], G["out_rceil_mx"])
    np.testing.assert_array_equal(G["gi_rceil_hp"], G["gi_rceil_mx"])
    assert not np.array_equal(G["gw_rceil_hp"], G["gw_rceil_mx"]) and not np.array_equal(G["out_floor_mx"], G["out_rceil_mx"])
    # the oracle's cast gives the reference's bytes for the four casts of the backward
    f = lambda key, *shape: _bf16(G[key]).float().numpy().reshape(*shape)  # noqa: E731
    for name, src in (("go", f("go", M, N)), ("go_t", f("go", M, N).T), ("x_t", f("x", M, K).T), ("w_t", f("w", N, K).T)):
        q, s = mx_ref.to_mx(np.ascontiguousarray(src), mx_ref.RCEIL)
        np.testing.assert_array_equal(q, G[name + "_q"])
        np.testing.assert_array_equal(s, G[name + "_s"])
