"""GPU: MXFP8 dense-linear training -- the one-pass rowwise + colwise cast against the two casts it replaces, byte for byte; the dense
weight-gradient entry against the grouped entry with one group; the autograd Function of _to_mxfp8_then_scaled_mm against hand-made casts
(bit-equal) and against the fixture written from the reference (tests/golden/mxfp8_linear_bwd.npz: the bound of
test_mxfp8_grouped_bwd_gpu.py, and the reference's SQNR bars); quantize_(model, MXFP8TrainingOpConfig()) against the same model built from
MXFP8Linear, and a wrapped expert parameter through torch._grouped_mm against the grouped entry called directly.

The C ABI cases of the cast write into guarded, poisoned buffers (tests/_parity.py).
Measured on an MI355X (the SQNR test prints its own): out 28.6 dB, grad_input 28.6 dB, grad_weight 28.5 dB, 55.6 dB with wgrad_with_hp
(profiles/pytest_gpu_mxfp8_linear_bwd.log); the reference's CPU run on the same inputs gives 28.58 / 28.55 / 28.51 / 55.63.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
from torch import nn

import _parity
from ao_amd import _lib, ops, torch_ops
from ao_amd.prototype import mx, mx_training as T
from ao_amd.quantization import KernelPreference, quantize_
from oracle import mx_ref
from test_route_parity_gpu import Draw

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
RCEIL, FLOOR = mx.ScaleCalculationMode.RCEIL, mx.ScaleCalculationMode.FLOOR
E4M3 = ops.MX_FMT_E4M3


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    return _load("make_golden_mxfp8_linear_bwd").load()


def _bf16(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f32(bits):
    return _bf16(bits).float().numpy()


def _u8(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _dev(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


# ---- the cast ----------------------------------------------------------------------------------------------------------------------------
def _cast_input(R, C, seed):
    """bf16 [R, C] whose 32 x 32 patches span 2^-30 .. 2^30, with (all inside the first 32 x 32 patch, so that every shape has them) an
    all-zero block in each direction, one NaN, one Inf, +448 2^10 and -448 2^-22 at the amax of their blocks, and a row of subnormals."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, C, generator=g, dtype=torch.float64)
    x = x * torch.exp2(torch.randint(-30, 31, (R // 32, C // 32), generator=g).double()).repeat_interleave(32, 0).repeat_interleave(32, 1)
    x[:32, :32] = torch.randn(32, 32, generator=g, dtype=torch.float64)
    x[0, :32] = 0.0   # a zero 1 x 32 block
    x[:32, 3] = 0.0   # a zero 32 x 1 block
    x[5, 7] = float("nan")
    x[9, 11] = float("inf")
    x[13, 17] = 448.0 * 2.0 ** 10
    x[20, :32] *= 2.0 ** -20
    x[20, 2] = -448.0 * 2.0 ** -22
    x = x.to(torch.bfloat16)
    sub = torch.arange(1, 33, dtype=torch.int16)  # bf16 subnormals: bit patterns 0x0001 .. 0x0020, every other one negative
    x.view(torch.int16)[25, :32] = sub | (torch.arange(32, dtype=torch.int16) % 2 * -32768).to(torch.int16)
    return x.to(DEV)


def _guarded_bytes(n):
    return _parity.Guarded(1, n // 2, torch.bfloat16, torch.device(DEV, 0))


def _bytes_of(buf, *shape):
    return buf.bits().contiguous().view(torch.uint8).reshape(*shape).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [RCEIL, FLOOR], ids=["rceil", "floor"])
@pytest.mark.parametrize("R,C", [(32, 32), (160, 96), (256, 384)], ids=["32x32", "160x96", "256x384"])
def test_the_one_pass_cast_writes_the_bytes_of_the_two_casts(R, C, mode):
    x = _cast_input(R, C, 100 + R + C)
    q, s = ops.mxfp8_quantize(x, mode)
    q_t, s_t = ops.mxfp8_quantize_colwise(x, mode)
    assert bool((s.view(torch.uint8) == 255).any()) and bool((s.view(torch.uint8)[0, 0] == 0))  # the NaN / Inf blocks and the zero block are there
    bq, bs, bqt, bst = _guarded_bytes(R * C), _guarded_bytes(R * C // 32), _guarded_bytes(R * C), _guarded_bytes(R * C // 32)
    _lib.check(_lib.lib().ao_mxfp8_quantize_rowcol(x.data_ptr(), bq.out.data_ptr(), bs.out.data_ptr(), bqt.out.data_ptr(), bst.out.data_ptr(),
                                                   R, C, ops.MX_SCALE_MODES[mode.value], torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for b in (bq, bs, bqt, bst):
        assert not b.guard_problems(), b.guard_problems()
    np.testing.assert_array_equal(_bytes_of(bq, R, C), _u8(q))
    np.testing.assert_array_equal(_bytes_of(bs, R, C // 32), _u8(s))
    np.testing.assert_array_equal(_bytes_of(bqt, C, R), _u8(q_t.t()))
    np.testing.assert_array_equal(_bytes_of(bst, R // 32, C), _u8(s_t.t()))
    # the op: the same bytes, and the views that mxfp8_quantize_colwise returns
    o = torch.ops.ao_mi355.mxfp8_quantize_rowcol(x, mode.value)
    for got, want in zip(o, (q, s, q_t, s_t)):
        assert got.dtype == want.dtype and got.shape == want.shape and got.stride() == want.stride()
        np.testing.assert_array_equal(_u8(got), _u8(want))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rceil", "floor"])
def test_torchao_mxfp8_quantize_with_both_flags_equals_one_flag_at_a_time(mode):
    assert torch_ops.load_ops_library()
    x = _cast_input(160, 96, 7)
    both = torch.ops.torchao.mxfp8_quantize(x, True, True, 32, 32, "e4m3", mode)
    rows = torch.ops.torchao.mxfp8_quantize(x, True, False, 32, 1, "e4m3", mode)
    cols = torch.ops.torchao.mxfp8_quantize(x, False, True, 1, 32, "e4m3", mode)
    for got, want in zip(both, (rows[0], cols[1], rows[2], cols[3])):  # (out_r, out_c, sc_r, sc_c)
        assert got.dtype == want.dtype and got.shape == want.shape and got.stride() == want.stride() and got.numel() > 0
        np.testing.assert_array_equal(got.view(torch.uint8).cpu().numpy(), want.view(torch.uint8).cpu().numpy())


@pytest.mark.gpu
def test_the_backwards_casts_equal_the_fixture():
    G = fixture()
    N, K = G["w"].shape
    go, x, w = (_bf16(G[k]).to(DEV) for k in ("go", "x", "w"))
    q, s, q_t, s_t = ops.mxfp8_quantize_rowcol(go.reshape(-1, N))
    for got, key in ((q, "go_q"), (s, "go_s"), (q_t.t(), "go_t_q"), (s_t, "go_t_s")):
        np.testing.assert_array_equal(_u8(got), G[key])
    q_t, s_t = ops.mxfp8_quantize_colwise(x.reshape(-1, K))
    np.testing.assert_array_equal(_u8(q_t.t()), G["x_t_q"])
    np.testing.assert_array_equal(_u8(s_t), G["x_t_s"])
    q_t, s_t = ops.mxfp8_quantize_colwise(w)  # the weight cast along N: codes [K][N], scales brought to [K][N/32]
    np.testing.assert_array_equal(_u8(q_t.t()), G["w_t_q"])
    np.testing.assert_array_equal(_u8(s_t), G["w_t_s"])


# ---- the dense weight gradient -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(96, 160, 288), (256, 128, 128)])
def test_dense_wgrad_has_the_bits_of_the_grouped_entry_with_one_group(M, N, K):
    d = Draw(5000 + M + N + K, torch.device(DEV, 0))
    g, gs, x, xs = d.fp8(N, M), d.e8m0(M // 32, N), d.fp8(K, M), d.e8m0(M // 32, K)
    want = ops.mxfp8_grouped_mm_wgrad(g, gs, x, xs, torch.tensor([M], dtype=torch.int32, device=DEV), N, K)
    got = torch.ops.ao_mi355.mxfp8_mm_wgrad(g, gs, x, xs, N, K)
    assert tuple(got.shape) == (N, K) and got.dtype == torch.bfloat16 and bool(got.any())
    np.testing.assert_array_equal(_bits(got), _bits(want[0]))


@pytest.mark.gpu
def test_dense_wgrad_of_no_tokens_is_zero():
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)  # noqa: E731
    out = ops.mxfp8_mm_wgrad(z(128, 0), z(0, 128), z(160, 0), z(0, 160), 128, 160)
    assert tuple(out.shape) == (128, 160) and not bool(out.view(torch.int16).any())


# ---- the Function ------------------------------------------------------------------------------------------------------------------------
def _strided(t):
    """The same values, non-contiguous (the reference's regression case for grad_out, mxfp8_linear.py:157-162)."""
    out = t.transpose(0, 1).contiguous().transpose(0, 1)
    assert not out.is_contiguous()
    return out


@functools.lru_cache(maxsize=None)
def run(mode=RCEIL, hp=False, freeze=None):
    """(out, grad_input, grad_weight) of one forward + backward on the fixture's tensors: a 3-D input, a non-contiguous grad_out."""
    G = fixture()
    x = _bf16(G["x"]).to(DEV).requires_grad_(freeze != "input")
    w = _bf16(G["w"]).to(DEV).requires_grad_(freeze != "weight")
    y = T._to_mxfp8_then_scaled_mm(x, w, KernelPreference.EMULATED, mode, hp)
    y.backward(_strided(_bf16(G["go"]).to(DEV)))
    assert y.dtype == torch.bfloat16 and y.shape == G["out_rceil_mx"].shape
    return y.detach(), x.grad, w.grad


@functools.lru_cache(maxsize=None)
def _mags(mode):
    """The oracle's sum |dq| |dq| behind every element of out [M, N], grad_input [M, K] and grad_weight [N, K]: its grouped mm, one group."""
    G = fixture()
    N, K = G["w"].shape
    x, w, go = _f32(G["x"]).reshape(-1, K), _f32(G["w"]), _f32(G["go"]).reshape(-1, N)
    m = mx_ref.RCEIL if mode == RCEIL else mx_ref.FLOOR
    cast = lambda v: mx_ref.to_mx(np.ascontiguousarray(v), m)  # noqa: E731
    one = lambda a, b: mx_ref.grouped_mm(*cast(a), *(v[None] for v in cast(b)), np.array([a.shape[0]]), return_abs=True)[1]  # noqa: E731
    return one(x, w), one(go, w.T), one(go.T, x.T)


def _within(y_bits, ref_bits, mag):
    y, ref = _f32(y_bits).astype(np.float64), _f32(ref_bits).astype(np.float64)
    return np.all(np.abs(y - ref) <= np.abs(ref) * 2.0 ** -7 + mag.reshape(ref.shape) * 2.0 ** -16)


def _sqnr(y, ref):
    return 10 * np.log10(np.sum(ref.astype(np.float64) ** 2) / np.sum((y.astype(np.float64) - ref) ** 2))


@pytest.mark.gpu
def test_grad_input_is_mx_mm_on_hand_made_casts():
    G = fixture()
    hand = ops.mx_mm(_dev(G["go_q"]), _dev(G["go_s"]), _dev(G["w_t_q"]), _dev(G["w_t_s"]), None, E4M3)
    gi = run()[1]
    assert gi.shape == G["x"].shape and gi.dtype == torch.bfloat16
    np.testing.assert_array_equal(_bits(gi).reshape(hand.shape), _bits(hand))


@pytest.mark.gpu
def test_grad_weight_is_the_wgrad_op_on_hand_made_casts():
    G = fixture()
    N, K = G["w"].shape
    hand = ops.mxfp8_mm_wgrad(_dev(G["go_t_q"]), _dev(G["go_t_s"].T), _dev(G["x_t_q"]), _dev(G["x_t_s"].T), N, K)
    np.testing.assert_array_equal(_bits(run()[2]), _bits(hand))


@pytest.mark.gpu
@pytest.mark.parametrize("one_pass", [True, False], ids=["one_pass", "two_launches"])
def test_either_cast_of_grad_out_gives_the_functions_bits(one_pass):
    """mx.ONE_PASS_CAST forces the one-pass cast of grad_out or the two launches (by default the tensor's size decides): the same
    gradients either way, from the dense Function and from the grouped one."""
    G = fixture()
    want = run()
    GG = _load("make_golden_mxfp8_bwd").load()
    offs, ggo = torch.from_numpy(GG["offs"]).to(DEV), _bf16(GG["go"]).to(DEV)
    assert mx.ONE_PASS_CAST is None
    grads = []
    for force in (one_pass, None):
        mx.ONE_PASS_CAST = force
        try:
            x, w = _bf16(G["x"]).to(DEV).requires_grad_(True), _bf16(G["w"]).to(DEV).requires_grad_(True)
            T._to_mxfp8_then_scaled_mm(x, w, KernelPreference.AUTO, RCEIL).backward(_bf16(G["go"]).to(DEV))
            a, e = _bf16(GG["a"]).to(DEV).requires_grad_(True), _bf16(GG["w"]).to(DEV).requires_grad_(True)
            mx._to_mxfp8_then_scaled_grouped_mm(a, e.transpose(-2, -1), offs).backward(ggo)
        finally:
            mx.ONE_PASS_CAST = None
        grads.append((x.grad, w.grad, a.grad, e.grad))
    np.testing.assert_array_equal(_bits(grads[0][0]), _bits(want[1]))
    np.testing.assert_array_equal(_bits(grads[0][1]), _bits(want[2]))
    for forced, default in zip(*grads):
        np.testing.assert_array_equal(_bits(forced), _bits(default))


@pytest.mark.gpu
def test_wgrad_with_hp_is_the_bf16_matmul():
    G = fixture()
    N, K = G["w"].shape
    go, x = _bf16(G["go"]).to(DEV).reshape(-1, N), _bf16(G["x"]).to(DEV).reshape(-1, K)
    _, gi, gw = run(hp=True)
    np.testing.assert_array_equal(_bits(gw), _bits(torch.mm(go.t(), x)))
    np.testing.assert_array_equal(_bits(gi), _bits(run()[1]))  # the grad_input does not depend on it


@pytest.mark.gpu
@pytest.mark.parametrize("tag,mode,hp", [("rceil_mx", RCEIL, False), ("rceil_hp", RCEIL, True), ("floor_mx", FLOOR, False)],
                         ids=["rceil_mx", "rceil_hp", "floor_mx"])
def test_the_function_stays_within_the_bound_of_the_fixture(tag, mode, hp):
    G = fixture()
    mag_o, mag_i, mag_w = _mags(mode)
    y, gi, gw = run(mode, hp)
    assert tuple(gi.shape) == G["x"].shape and tuple(gw.shape) == G["w"].shape
    assert _within(_bits(y), G["out_" + tag], mag_o)
    assert _within(_bits(gi), G["gi_" + tag], mag_i)
    assert _within(_bits(gw), G["gw_" + tag], mag_w)


@pytest.mark.gpu
def test_sqnr_against_fp32_matmuls_meets_the_references_bars():
    """test_mxfp8_linear.py:73-90: >= 27 dB on the output, 25 dB on the input gradient, 24 dB on the weight gradient, 34 dB with wgrad_with_hp."""
    G = fixture()
    N, K = G["w"].shape
    x, w, go = _f32(G["x"]).reshape(-1, K), _f32(G["w"]), _f32(G["go"]).reshape(-1, N)
    y, gi, gw = run()
    got = [_sqnr(_f32(_bits(t)).reshape(r.shape), r) for t, r in ((y, x @ w.T), (gi, go @ w), (gw, go.T @ x), (run(hp=True)[2], go.T @ x))]
    print("SQNR vs fp32: out %.2f dB, grad_input %.2f dB, grad_weight %.2f dB, %.2f dB with wgrad_with_hp" % tuple(got))
    assert got[0] >= 27.0 and got[1] >= 25.0 and got[2] >= 24.0 and got[3] >= 34.0


@pytest.mark.gpu
def test_a_frozen_operand_skips_its_gradient():
    y, gi, gw = run(freeze="weight")
    assert gw is None
    np.testing.assert_array_equal(_bits(gi), _bits(run()[1]))
    y, gi, gw = run(freeze="input")
    assert gi is None
    np.testing.assert_array_equal(_bits(gw), _bits(run()[2]))
    # and no launch: the skipped side's ops are never called
    G = fixture()
    calls = []
    real_wgrad, real_mm = ops.mxfp8_mm_wgrad, ops.mx_mm
    ops.mxfp8_mm_wgrad = lambda *a, **k: calls.append("wgrad") or real_wgrad(*a, **k)
    ops.mx_mm = lambda *a, **k: calls.append("dgrad") or real_mm(*a, **k)
    try:
        for freeze, want in (("weight", ["dgrad"]), ("input", ["wgrad"])):
            x = _bf16(G["x"]).to(DEV).requires_grad_(freeze != "input")
            w = _bf16(G["w"]).to(DEV).requires_grad_(freeze != "weight")
            y = T._to_mxfp8_then_scaled_mm(x, w, KernelPreference.AUTO, RCEIL)
            del calls[:]  # (the forward's ops.mx_linear runs ops.mx_mm itself at this size)
            y.backward(_bf16(G["go"]).to(DEV))
            assert calls == want, (freeze, calls)
    finally:
        ops.mxfp8_mm_wgrad, ops.mx_mm = real_wgrad, real_mm


@pytest.mark.gpu
def test_a_call_under_no_grad_has_mx_linears_bits():
    G = fixture()
    N, K = G["w"].shape
    x, w = _bf16(G["x"]).to(DEV).requires_grad_(True), _bf16(G["w"]).to(DEV).requires_grad_(True)
    with torch.no_grad():
        quiet = T._to_mxfp8_then_scaled_mm(x, w, KernelPreference.AUTO, RCEIL)
    assert not quiet.requires_grad and quiet.shape == G["out_rceil_mx"].shape
    w_q, w_s = ops.mxfp8_quantize(w.detach(), RCEIL)
    plain = ops.mx_linear(x.detach().reshape(-1, K), w_q, w_s, None, E4M3, RCEIL)
    np.testing.assert_array_equal(_bits(quiet).reshape(-1, N), _bits(plain))
    np.testing.assert_array_equal(_bits(quiet), _bits(run()[0]))  # and the Function's forward is that call


# ---- quantize_ ---------------------------------------------------------------------------------------------------------------------------
def _two_layers(linear):
    torch.manual_seed(0)
    plain = nn.Sequential(nn.Linear(288, 160, bias=True), nn.Linear(160, 64, bias=False)).to(torch.bfloat16)
    model = nn.Sequential(linear(288, 160, bias=True), linear(160, 64, bias=False)).to(torch.bfloat16)
    model.load_state_dict(plain.state_dict())
    return model.to(DEV)


@pytest.mark.gpu
def test_quantize_gives_the_bits_of_the_model_built_from_mxfp8linear():
    G = fixture()
    ref, model = _two_layers(T.MXFP8Linear), _two_layers(nn.Linear)
    quantize_(model, T.MXFP8TrainingOpConfig())
    W = T.MXFP8TrainingWeightWrapperTensor
    assert all(type(p.data) is W and p.requires_grad for p in model.parameters()) and len(list(model.parameters())) == 3
    torch.manual_seed(1)
    go = torch.randn(2, 48, 64, device=DEV).to(torch.bfloat16)
    outs = []
    for m in (ref, model):
        x = _bf16(G["x"]).to(DEV).requires_grad_(True)
        y = m(x)
        y.backward(go)
        outs.append((y, x.grad))
    assert type(outs[1][0]) is torch.Tensor and outs[1][0].dtype == torch.bfloat16
    np.testing.assert_array_equal(_bits(outs[1][0]), _bits(outs[0][0]))
    np.testing.assert_array_equal(_bits(outs[1][1]), _bits(outs[0][1]))
    for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and type(p.grad) is torch.Tensor and bool(p.grad.any()), name
        np.testing.assert_array_equal(_bits(p.grad), _bits(q.grad), err_msg=name)
    # one optimizer step changes the wrapped parameters' inner tensors, as it changes the plain model's
    before = [p.data._data.clone() for p in model.parameters()]
    torch.optim.SGD(model.parameters(), lr=0.5).step()
    torch.optim.SGD(ref.parameters(), lr=0.5).step()
    for b, p, q in zip(before, model.parameters(), ref.parameters()):
        assert type(p.data) is W and not torch.equal(b, p.data._data)
        np.testing.assert_array_equal(_bits(p.data._data), _bits(q.data))


@pytest.mark.gpu
def test_a_wrapped_expert_parameter_through_grouped_mm_has_the_grouped_entrys_bits():
    G = _load("make_golden_mxfp8_bwd").load()
    offs, go = torch.from_numpy(G["offs"]).to(DEV), _bf16(G["go"]).to(DEV)
    a1, w1 = _bf16(G["a"]).to(DEV).requires_grad_(True), _bf16(G["w"]).to(DEV).requires_grad_(True)
    y1 = mx._to_mxfp8_then_scaled_grouped_mm(a1, w1.transpose(-2, -1), offs)
    y1.backward(go)

    class Experts(nn.Module):
        def __init__(self):
            super().__init__()
            self.w = nn.Parameter(_bf16(G["w"]).to(DEV))

    experts = Experts()
    quantize_(experts, T.MXFP8TrainingOpConfig(), filter_fn=lambda mod, fqn: isinstance(mod, Experts))
    assert type(experts.w.data) is T.MXFP8TrainingWeightWrapperTensor and experts.w.ndim == 3
    a2 = _bf16(G["a"]).to(DEV).requires_grad_(True)
    y2 = torch._grouped_mm(a2, experts.w.transpose(-2, -1), offs=offs)
    y2.backward(go)
    assert type(y2) is torch.Tensor
    np.testing.assert_array_equal(_bits(y2), _bits(y1))
    np.testing.assert_array_equal(_bits(a2.grad), _bits(a1.grad))
    np.testing.assert_array_equal(_bits(experts.w.grad), _bits(w1.grad))
