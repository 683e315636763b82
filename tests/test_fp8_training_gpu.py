"""GPU: float8 training -- the HIP training casts against the numpy restatement (tests/fp8_training_ref.py, itself pinned to the fixture
written from the reference), byte for byte; the one-pass forms against the two-call forms; the autograd Function of Float8Linear against
ops.fp8_scaled_mm on hand-made casts (bit-equal) and against the reference's recorded run (tests/golden/fp8_training.npz: the bound of
test_mxfp8_linear_bwd_gpu.py, and the reference's SQNR bars); frozen operands, no_grad and convert_to_float8_training.

The C ABI case of the cast writes into guarded, poisoned buffers (tests/_parity.py).
Measured on an MI355X (the SQNR test prints its own; profiles/pytest_gpu_fp8_training.log): see the SQNR test's docstring.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
from torch import nn

import _parity
import fp8_training_ref as R
from ao_amd import _lib, ops
from ao_amd.float8 import CastConfig, Float8LinearConfig, convert_to_float8_training, e4m3_dtype
from ao_amd.float8.float8_linear import Float8Linear, LinearMMConfig, matmul_with_hp_or_float8_args

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
CONFIGS = {
    "rowwise": Float8LinearConfig.from_recipe_name("rowwise"),
    "rowwise_with_gw_hp": Float8LinearConfig.from_recipe_name("rowwise_with_gw_hp"),
    "tensorwise_e4m3": Float8LinearConfig(cast_config_grad_output=CastConfig(target_dtype=e4m3_dtype)),
}


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    return _load("make_golden_fp8_training").load()


def _bf16(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f32(bits):
    return _bf16(bits).float().numpy()


def _u8(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _u32(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t, dtype=np.float32)).view(np.uint32).reshape(-1)


# ---- the casts -------------------------------------------------------------------------------------------------------------------------
SHAPES = {"x_80x272": "x", "go_80x144": "go", "w_144x272": "w", "edge_80x48": "edge", "16x16": (16, 16), "1040x48": (1040, 48),
          "2064x48": (2064, 48)}  # 1040 rows: 9 row tiles of 128 merge into one column amax; 2064: 17


@functools.lru_cache(maxsize=None)
def cast_case(name):
    """(bf16 bits [R, C], {(axis, pow2): (codes, scale, inv_scale)} from the restatement), made once per shape."""
    src = SHAPES[name]
    if isinstance(src, str):
        xb = fixture()[src]
        xb = xb.reshape(-1, xb.shape[-1])
    else:
        g = torch.Generator().manual_seed(1000 + src[0])
        x = torch.randn(*src, generator=g) * torch.exp2(torch.randint(-12, 13, (src[0], 1), generator=g).float())
        xb = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return xb, {(ax, p): R.cast(xb, ax, bool(p)) for ax in (-1, 0, None) for p in (0, 1)}


def _same(got, want, transposed=False):
    """An op's (q, scale, inv_scale) against the restatement's; transposed: the op's codes are [C, R]."""
    q, s, inv = got
    wq, ws, winv = want
    n = q.shape[0]
    assert q.dtype == torch.float8_e4m3fn and s.dtype == inv.dtype == torch.float32 and tuple(s.shape) == tuple(inv.shape) == (n, 1)
    np.testing.assert_array_equal(_u8(q), wq.T if transposed else wq)
    np.testing.assert_array_equal(_u32(s), np.broadcast_to(_u32(ws), (n,)))  # a tensorwise scale fills the vector
    np.testing.assert_array_equal(_u32(inv), np.broadcast_to(_u32(winv), (n,)))


@pytest.mark.gpu
@pytest.mark.parametrize("pow2", [0, 1], ids=["plain", "pow2"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_cast_op_equals_the_restatement(name, pow2):
    xb, ref = cast_case(name)
    R_, C = xb.shape
    x = _bf16(xb).to(DEV)
    ra, ca = ops.fp8_train_amax(x, rows=True, cols=True)
    a = np.abs(_f32(xb))
    np.testing.assert_array_equal(_u32(ra), _u32(a.max(axis=1)))
    np.testing.assert_array_equal(_u32(ca), _u32(a.max(axis=0)))
    assert ops.fp8_train_amax(x, rows=False, cols=True)[0] is None and ops.fp8_train_amax(x)[1] is None
    np.testing.assert_array_equal(_u32(ops.fp8_train_amax(x, rows=False, cols=True)[1]), _u32(ca))
    # axiswise
    _same(ops.fp8_train_quantize_rowwise(x, pow2), ref[(-1, pow2)])
    _same(ops.fp8_train_quantize_colwise_t(x, pow2), ref[(0, pow2)], transposed=True)
    rows, cols = ops.fp8_train_quantize_both(x, pow2)
    _same(rows, ref[(-1, pow2)])
    _same(cols, ref[(0, pow2)], transposed=True)
    rows, cols = ops.fp8_train_cast(x, row_amax=ra, pow2=pow2)
    assert cols is None
    _same(rows, ref[(-1, pow2)])
    # tensorwise, either layout from the one amax
    t = ra.amax()
    rows, cols = ops.fp8_train_cast(x, t, t, pow2)
    _same(rows, ref[(None, pow2)])
    _same(cols, ref[(None, pow2)], transposed=True)
    _same(ops.fp8_train_quantize_colwise_t(x, pow2, amax=t), ref[(None, pow2)], transposed=True)
    # mixed: rows axiswise, columns tensorwise
    rows, cols = ops.fp8_train_cast(x, ra, t, pow2)
    _same(rows, ref[(-1, pow2)])
    _same(cols, ref[(None, pow2)], transposed=True)


@pytest.mark.gpu
def test_a_row_count_that_is_no_multiple_of_16_casts_rowwise_only():
    xb, _ = cast_case("go_80x144")
    xb = xb[:41]
    x = _bf16(xb).to(DEV)
    for pow2 in (0, 1):
        _same(ops.fp8_train_quantize_rowwise(x, pow2), R.cast(xb, -1, bool(pow2)))
        _same(ops.fp8_train_cast(x, ops.fp8_train_amax(x)[0], None, pow2)[0], R.cast(xb, -1, bool(pow2)))
    with pytest.raises(ValueError, match="R=41 must be a multiple of 16"):
        ops.fp8_train_quantize_colwise_t(x)
    with pytest.raises(ValueError, match="C=24 must be a multiple of 16"):
        ops.fp8_train_quantize_rowwise(x[:, :24])
    q, s, inv = ops.fp8_train_quantize_rowwise(x[:0])
    assert tuple(q.shape) == (0, 144) and tuple(s.shape) == (0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["x_80x272", "1040x48"])
def test_the_c_entry_points_stay_inside_their_outputs_and_agree_with_each_other(name):
    """Guarded, poisoned buffers: the one-pass cast writes exactly the bytes of the row call and the column call, the one-launch row cast
    exactly those of amax + cast, and nothing outside."""
    xb, ref = cast_case(name)
    R_, C = xb.shape
    x = _bf16(xb).to(DEV)
    dev = torch.device(DEV, 0)
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    G = lambda n, dt=torch.float32: _parity.Guarded(1, n, dt, dev)  # noqa: E731
    B = lambda n: _parity.Guarded(1, n // 2, torch.bfloat16, dev)  # noqa: E731  (n bytes)
    ra, ca = G(R_), G(C)
    _lib.check(lib.ao_fp8_train_amax(x.data_ptr(), ra.out.data_ptr(), ca.out.data_ptr(), R_, C, st))
    q, s, inv, qt, sc, invc = B(R_ * C), G(R_), G(R_), B(R_ * C), G(C), G(C)
    _lib.check(lib.ao_fp8_train_cast(x.data_ptr(), ra.out.data_ptr(), 1, ca.out.data_ptr(), 1, 1, q.out.data_ptr(), s.out.data_ptr(),
                                     inv.out.data_ptr(), qt.out.data_ptr(), sc.out.data_ptr(), invc.out.data_ptr(), R_, C, st))
    q1, s1, inv1 = B(R_ * C), G(R_), G(R_)
    _lib.check(lib.ao_fp8_train_quantize_rowwise(x.data_ptr(), q1.out.data_ptr(), s1.out.data_ptr(), inv1.out.data_ptr(), 1, R_, C, st))
    q2, s2, inv2 = B(R_ * C), G(C), G(C)
    _lib.check(lib.ao_fp8_train_cast(x.data_ptr(), None, 1, ca.out.data_ptr(), 1, 1, None, None, None, q2.out.data_ptr(), s2.out.data_ptr(),
                                     inv2.out.data_ptr(), R_, C, st))
    torch.cuda.synchronize()
    for b in (ra, ca, q, s, inv, qt, sc, invc, q1, s1, inv1, q2, s2, inv2):
        assert not b.guard_problems(), b.guard_problems()
    by = lambda b: b.bits().contiguous().view(torch.uint8).reshape(-1).cpu().numpy()  # noqa: E731
    wq, ws, winv = ref[(-1, 1)]
    np.testing.assert_array_equal(by(q).reshape(R_, C), wq)
    np.testing.assert_array_equal(by(s).view(np.uint32), _u32(ws))
    np.testing.assert_array_equal(by(inv).view(np.uint32), _u32(winv))
    np.testing.assert_array_equal(by(qt).reshape(C, R_), ref[(0, 1)][0].T)
    for one, two in ((q1, q), (s1, s), (inv1, inv), (q2, qt), (s2, sc), (inv2, invc)):
        np.testing.assert_array_equal(by(one), by(two))


@pytest.mark.gpu
def test_the_amax_and_the_cast_can_be_captured_in_a_graph():
    xb, ref = cast_case("w_144x272")
    x = _bf16(xb).to(DEV)
    ops.fp8_train_quantize_both(x, True)  # warm: the allocator's pools
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rows, cols = ops.fp8_train_quantize_both(x, True)
        g.replay()
    torch.cuda.synchronize()
    _same(rows, ref[(-1, 1)])
    _same(cols, ref[(0, 1)], transposed=True)


# ---- the Function ------------------------------------------------------------------------------------------------------------------------
def _strided(t):
    """The same values, non-contiguous."""
    out = t.transpose(0, 1).contiguous().transpose(0, 1)
    assert not out.is_contiguous()
    return out


def _operands(freeze=None):
    G = fixture()
    x = _bf16(G["x"]).to(DEV).requires_grad_(freeze != "input")
    w = _bf16(G["w"]).to(DEV).requires_grad_(freeze != "weight")
    return x, w, _bf16(G["go"]).to(DEV)


@functools.lru_cache(maxsize=None)
def run(tag="rowwise", freeze=None):
    """(out, grad_input, grad_weight) of one forward + backward on the fixture's tensors: a 3-D input, a non-contiguous grad_out."""
    x, w, go = _operands(freeze)
    y = matmul_with_hp_or_float8_args.apply(x, w.t(), LinearMMConfig(), CONFIGS[tag])
    y.backward(_strided(go))
    assert y.dtype == torch.bfloat16 and y.shape == fixture()["out_rowwise"].shape
    return y.detach(), x.grad, w.grad


@pytest.mark.gpu
def test_the_functions_casts_equal_the_fixture():
    """The operands of the three GEMMs, taken through the ops as the Function takes them, are the reference's recorded casts."""
    G = fixture()
    N, K = G["w"].shape
    x, w, go = (_bf16(G[k]).to(DEV) for k in ("x", "w", "go"))
    x, go = x.reshape(-1, K), go.reshape(-1, N)
    for pow2 in (0, 1):
        for name, t in (("x", x), ("w", w), ("go", go)):
            rows, cols = ops.fp8_train_quantize_both(t, pow2)
            for tag, (q, s, _), tr in (("r", rows, False), ("c", cols, True)):
                key = "%s_%s%d" % (name, tag, pow2)
                np.testing.assert_array_equal(_u8(q.t() if tr else q), G[key + "_q"], err_msg=key)
                np.testing.assert_array_equal(_u32(s), _u32(G[key + "_s"]), err_msg=key)
            tam = ops.fp8_train_amax(t)[0].amax()
            rows, cols = ops.fp8_train_cast(t, tam, tam, pow2)
            key = "%s_t%d" % (name, pow2)
            np.testing.assert_array_equal(_u8(rows[0]), G[key + "_q"], err_msg=key)
            np.testing.assert_array_equal(_u8(cols[0].t()), G[key + "_q"], err_msg=key)
            assert np.all(_u32(rows[1]) == _u32(G[key + "_s"])[0]) and np.all(_u32(cols[1]) == _u32(G[key + "_s"])[0])


@pytest.mark.gpu
def test_rowwise_is_fp8_scaled_mm_on_hand_made_casts():
    G = fixture()
    N, K = G["w"].shape
    x, w, go = (_bf16(G[k]).to(DEV) for k in ("x", "w", "go"))
    x, go = x.reshape(-1, K), go.reshape(-1, N)
    y, gi, gw = run("rowwise")
    xq, _, xi = ops.fp8_train_quantize_rowwise(x, True)
    wq, _, wi = ops.fp8_train_quantize_rowwise(w, True)
    np.testing.assert_array_equal(_bits(y).reshape(-1, N), _bits(ops.fp8_scaled_mm(xq, wq.t(), xi, wi)))
    gq, _, gi_ = ops.fp8_train_quantize_rowwise(go, True)
    wt, _, wti = ops.fp8_train_quantize_colwise_t(w, True)  # [K][N], one scale per k
    assert tuple(wt.shape) == (K, N)
    np.testing.assert_array_equal(_bits(gi).reshape(-1, K), _bits(ops.fp8_scaled_mm(gq, wt.t(), gi_, wti)))
    gt, _, gti = ops.fp8_train_quantize_colwise_t(go, True)  # [N][M]
    xt, _, xti = ops.fp8_train_quantize_colwise_t(x, True)   # [K][M]
    assert tuple(gw.shape) == (N, K) and gw.dtype == torch.bfloat16
    np.testing.assert_array_equal(_bits(gw), _bits(ops.fp8_scaled_mm(gt, xt.t(), gti, xti)))


@pytest.mark.gpu
def test_rowwise_with_gw_hp_keeps_grad_weight_in_bf16_and_scales_the_weight_tensorwise():
    G = fixture()
    N, K = G["w"].shape
    x, w, go = (_bf16(G[k]).to(DEV) for k in ("x", "w", "go"))
    x, go = x.reshape(-1, K), go.reshape(-1, N)
    y, gi, gw = run("rowwise_with_gw_hp")
    np.testing.assert_array_equal(_bits(gw), _bits(torch.mm(go.t(), x)))
    np.testing.assert_array_equal(_bits(y), _bits(run("rowwise")[0]))
    gq, _, gi_ = ops.fp8_train_quantize_rowwise(go, True)
    wt, ws, wti = ops.fp8_train_quantize_colwise_t(w, True, amax=ops.fp8_train_amax(w)[0].amax())
    assert tuple(wti.shape) == (K, 1) and len(set(_u32(wti).tolist())) == 1  # the one scale, broadcast to the vector the GEMM takes
    np.testing.assert_array_equal(_bits(gi).reshape(-1, K), _bits(ops.fp8_scaled_mm(gq, wt.t(), gi_, wti)))


@functools.lru_cache(maxsize=None)
def _mags(tag):
    """sum |dq(a)| |dq(b)| behind every element of out [M, N], grad_input [M, K] and grad_weight [N, K], from the restatement's casts of
    the operands as the config casts them (float64); the bf16 grad_weight of rowwise_with_gw_hp: sum |go| |x|."""
    G = fixture()
    N, K = G["w"].shape
    xb, wb, gb = G["x"].reshape(-1, K), G["w"], G["go"].reshape(-1, N)
    c = CONFIGS[tag]
    p = c.round_scales_to_power_of_2

    def dq(b, cc, axis):
        if cc.scaling_type.value == "disabled":
            return np.abs(_f32(b).astype(np.float64))
        q, s, _ = R.cast(b, axis if cc.scaling_granularity.value == "axiswise" else None, p)
        return np.abs(R.dequant(q, s))

    mag_o = dq(xb, c.cast_config_input, 1) @ dq(wb, c.cast_config_weight, 1).T
    mag_i = dq(gb, c.cast_config_grad_output, 1) @ dq(wb, c.cast_config_weight_for_grad_input, 0)
    mag_w = dq(gb, c.cast_config_grad_output_for_grad_weight, 0).T @ dq(xb, c.cast_config_input_for_grad_weight, 0)
    return mag_o, mag_i, mag_w


def _within(y_bits, ref_bits, mag):
    y, ref = _f32(y_bits).astype(np.float64), _f32(ref_bits).astype(np.float64)
    return np.all(np.abs(y - ref) <= np.abs(ref) * 2.0 ** -7 + mag.reshape(ref.shape) * 2.0 ** -16)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CONFIGS))
def test_the_function_stays_within_the_bound_of_the_fixture(tag):
    """|y - ref| <= |ref| 2^-7 + mag 2^-16 against the reference's recorded CPU run, for out, grad_input and grad_weight."""
    G = fixture()
    mag_o, mag_i, mag_w = _mags(tag)
    y, gi, gw = run(tag)
    assert tuple(gi.shape) == G["x"].shape and tuple(gw.shape) == G["w"].shape
    assert _within(_bits(y), G["out_" + tag], mag_o)
    assert _within(_bits(gi), G["gi_" + tag], mag_i)
    assert _within(_bits(gw), G["gw_" + tag], mag_w)


def _sqnr(y, ref):
    return 10 * np.log10(np.sum(ref.astype(np.float64) ** 2) / np.sum((y.astype(np.float64) - ref) ** 2))


@pytest.mark.gpu
def test_sqnr_against_fp32_matmuls_meets_the_references_bars():
    """test/float8/test_base.py:313-319: >= 18 dB on the output, >= 17 dB on grad_weight; the same 17 dB on grad_input.
    Measured on an MI355X: out 28.37 dB, grad_input 28.49 dB, grad_weight 28.48 dB (the reference's CPU run: 28.37 / 28.49 / 28.48)."""
    G = fixture()
    N, K = G["w"].shape
    x, w, go = _f32(G["x"]).reshape(-1, K), _f32(G["w"]), _f32(G["go"]).reshape(-1, N)
    y, gi, gw = run("rowwise")
    got = [_sqnr(_f32(_bits(t)).reshape(r.shape), r) for t, r in ((y, x @ w.T), (gi, go @ w), (gw, go.T @ x))]
    print("SQNR vs fp32 (rowwise): out %.2f dB, grad_input %.2f dB, grad_weight %.2f dB" % tuple(got))
    assert got[0] >= 18.0 and got[1] >= 17.0 and got[2] >= 17.0


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CONFIGS))
def test_a_frozen_operand_skips_its_gradient_and_its_casts(tag):
    full = run(tag)
    y, gi, gw = run(tag, freeze="weight")
    assert gw is None
    np.testing.assert_array_equal(_bits(gi), _bits(full[1]))
    np.testing.assert_array_equal(_bits(y), _bits(full[0]))
    y, gi, gw = run(tag, freeze="input")
    assert gi is None
    np.testing.assert_array_equal(_bits(gw), _bits(full[2]))
    # and no launch for the skipped side: count the transposed outputs the backward's casts make
    calls = []
    real = ops.fp8_train_cast
    ops.fp8_train_cast = lambda t, ra=None, ca=None, pow2=False: calls.append((tuple(t.shape), ra is not None, ca is not None)) or real(t, ra, ca, pow2)
    try:
        for freeze in ("weight", "input"):
            x, w, go = _operands(freeze)
            y = matmul_with_hp_or_float8_args.apply(x, w.t(), LinearMMConfig(), CONFIGS[tag])
            del calls[:]
            y.backward(go)
            M, N, K = 80, 144, 272
            if freeze == "weight":  # grad_input only: no cast of x, grad_out not cast along dim 0
                assert not any(shape == (M, K) for shape, _, _ in calls) and not any(shape == (M, N) and cols for shape, _, cols in calls), calls
            else:  # grad_weight only: no cast of W, grad_out not cast along dim -1
                assert not any(shape == (N, K) for shape, _, _ in calls) and not any(shape == (M, N) and rows for shape, rows, _ in calls), calls
    finally:
        ops.fp8_train_cast = real


@pytest.mark.gpu
def test_a_call_under_no_grad_has_the_forwards_bits():
    x, w, _ = _operands()
    with torch.no_grad():
        quiet = matmul_with_hp_or_float8_args.apply(x, w.t(), LinearMMConfig(), CONFIGS["rowwise"])
    assert not quiet.requires_grad
    np.testing.assert_array_equal(_bits(quiet), _bits(run("rowwise")[0]))
    # M = 40 (no multiple of 16) is accepted where no grad_weight is computed
    with torch.no_grad():
        part = matmul_with_hp_or_float8_args.apply(x[:1], w.t(), LinearMMConfig(), CONFIGS["rowwise"])
    # rowwise: a row's output depends on that row alone (up to the summation order of the GEMM form the other M selects)
    assert tuple(part.shape) == (1, 40, 144) and torch.allclose(part.float(), quiet[:1].float(), rtol=2.0 ** -7, atol=2.0 ** -10)


# ---- model conversion --------------------------------------------------------------------------------------------------------------------
def _two_layers():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(272, 144, bias=True), nn.Linear(144, 64, bias=False)).to(torch.bfloat16).to(DEV)


@pytest.mark.gpu
def test_convert_gives_the_bits_of_the_model_built_by_hand():
    cfg = CONFIGS["rowwise"]
    model, plain = _two_layers(), _two_layers()
    out = convert_to_float8_training(model, module_filter_fn=lambda m, fqn: fqn != "1", config=cfg)
    assert out is model and type(model[0]) is Float8Linear and type(model[1]) is nn.Linear
    ref = nn.Sequential(Float8Linear.from_float(plain[0], cfg), plain[1])
    x0 = _operands()[0].detach()
    torch.manual_seed(1)
    go = torch.randn(2, 40, 64, device=DEV).to(torch.bfloat16)
    outs = []
    for m in (ref, model):
        x = x0.clone().requires_grad_(True)
        y = m(x)
        y.backward(go)
        outs.append((y, x.grad))
    assert outs[1][0].dtype == torch.bfloat16 and tuple(outs[1][0].shape) == (2, 40, 64)
    np.testing.assert_array_equal(_bits(outs[1][0]), _bits(outs[0][0]))
    np.testing.assert_array_equal(_bits(outs[1][1]), _bits(outs[0][1]))
    for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and bool(p.grad.any()), name
        np.testing.assert_array_equal(_bits(p.grad), _bits(q.grad), err_msg=name)
    # the bias is added in bf16 outside the GEMM
    h = matmul_with_hp_or_float8_args.apply(x0, model[0].weight.t(), model[0].linear_mm_config, cfg)
    np.testing.assert_array_equal(_bits(model[0](x0)), _bits(h + model[0].bias))
    assert not torch.equal(h, model[0](x0))
