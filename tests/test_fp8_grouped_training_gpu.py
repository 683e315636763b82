"""GPU: float8 rowwise training of the MoE grouped GEMM -- the jagged and the 3-D transposing casts bit for bit against the numpy
restatement (tests/fp8_grouped_training_ref.py) and the fixture written from the reference (tests/golden/fp8_grouped_training.npz); the
weight-gradient GEMM through the C ABI against a float64 oracle in guarded buffers (tests/_parity.py); the autograd Function.

The wgrad bound is the one of the other 8-bit GEMM route tests, |y - ref| <= ulp + 2 max(K, floor) 2^-24 S, with S = sum |dq g| |dq x|
(the scale product applied), K the group's token count and the floor and equal fraction of the scaled e4m3 MFMA, the instruction this
kernel issues with unit block scales (test_route_parity_gpu.K_FLOOR_E4M3_MX = 1408, EQUAL_GROUPED_MX = 0.96).
The Function is held to |y - ref| <= |ref| 2^-7 + mag 2^-16 of the recording, mag = sum |dq a| |dq b| (test_fp8_training_gpu._within): both
sides round once to bf16 (2^-8 |ref| each) and fp32 accumulation over at most 256 terms costs at most 256 x 2^-24 = 2^-16 of mag; the
fixture's contractions are 128, 128 and <= 160 terms.
Measured on an MI355X (each test prints its own; profiles/pytest_gpu_fp8_grouped_training.log): the worst wgrad element needs
max(K, floor) >= 110; 99.0 - 99.1 % of the Function's outputs have the recording's bits; SQNR against fp32 matmuls 28.50 / 28.49 /
28.45 dB (out / grad_A / grad_B), 28.48 / 28.52 / 28.47 dB with padded groups.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
from torch import nn

import _parity
import fp8_grouped_training_ref as R
from ao_amd import _lib, ops
from ao_amd.prototype import fp8_grouped_training as FG
from ao_amd.prototype.fp8_grouped_training import (Float8TrainingOpConfig, _to_fp8_rowwise_then_scaled_grouped_mm)
from ao_amd.prototype.mx import pad_token_groups
from ao_amd.quantization.quant_api import quantize_
from test_route_parity_grouped_gpu import EQUAL_GROUPED_MX
from test_route_parity_gpu import K_FLOOR_E4M3_MX

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MAKER = _load("make_golden_fp8_grouped_training")


@functools.lru_cache(maxsize=None)
def fixture():
    return MAKER.load()


def _bf16(bits_):
    return torch.from_numpy(np.ascontiguousarray(bits_).view(np.int16).copy()).view(torch.bfloat16)


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def _f32(bits_):
    return R.bf16.from_bits(bits_)


def _u8(t):
    return t.detach().contiguous().cpu().view(torch.uint8).numpy()


def _u32(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float32)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)
    return t.view(dtype) if dtype is not None else t


def _randn_bits(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return _bits((torch.randn(*shape, generator=g) * scale).to(torch.bfloat16))


# ---- the jagged cast ---------------------------------------------------------------------------------------------------------------------
JAGGED = {
    "256x144": ((256, 144), [48, 48, 208, 240]),   # an empty group, a tail of 16 unowned rows, a partial column tile
    "400x272": ((400, 272), [16, 400]),            # one group over four row tiles merging into one amax, a partial row tile
    "16x16": ((16, 16), [0, 0, 16]),
}


def _check_jagged(xb, offs, pow2):
    q_t, s, inv = ops.fp8_train_quantize_group_colwise_t(_bf16(xb).to(DEV), _dev(np.asarray(offs, dtype=np.int32)), bool(pow2))
    torch.cuda.synchronize()
    rq, rs, rinv = R.group_colwise(xb, offs, bool(pow2))
    assert q_t.dtype == torch.float8_e4m3fn and tuple(q_t.shape) == xb.shape[::-1] and q_t.is_contiguous()
    assert tuple(s.shape) == tuple(inv.shape) == (len(offs), xb.shape[1]) and s.dtype == inv.dtype == torch.float32
    np.testing.assert_array_equal(_u32(s), _u32(rs))
    np.testing.assert_array_equal(_u32(inv), _u32(rinv))
    np.testing.assert_array_equal(_u8(q_t).T, rq)
    return q_t, s, inv


@pytest.mark.parametrize("pow2", [0, 1])
@pytest.mark.parametrize("case", list(JAGGED))
def test_the_jagged_cast_equals_the_restatement(case, pow2):
    shape, offs = JAGGED[case]
    q_t, s, _ = _check_jagged(_randn_bits(shape, 7 + shape[0]), offs, pow2)
    if case == "256x144":
        assert not _u8(q_t)[:, 240:].any() and np.all(_u32(s[1]) == _u32(R.T.amax_to_scale(np.zeros(1, np.float32), bool(pow2)))[0])


@pytest.mark.parametrize("pow2", [0, 1])
def test_the_jagged_cast_of_the_edge_tensor(pow2):
    """A column that is all zero inside one group only, the largest finite bf16 in one group only, one 1e-20."""
    offs = [32, 64, 96]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(96, 48, generator=g)
    x[32:64, 5] = 0.0
    x[40, 11] = torch.finfo(torch.bfloat16).max
    x[70, 9] = 1e-20
    xb = _bits(x.to(torch.bfloat16))
    q_t, s, _ = _check_jagged(xb, offs, pow2)
    s = s.cpu().numpy()
    zero_scale = R.T.amax_to_scale(np.zeros(1, np.float32), bool(pow2))[0]
    assert s[1, 5] == zero_scale and s[0, 5] != zero_scale and s[2, 5] != zero_scale and not _u8(q_t)[5, 32:64].any()
    # the largest bf16 lands on 448, or (255 x a power of two) on 256 under the scale rounded down ...
    assert _u8(q_t)[11, 40] == (0x78 if pow2 else 0x7E) and s[1, 11] < 1e-30
    plain = R.group_colwise(_bits(torch.randn(96, 48, generator=torch.Generator().manual_seed(11)).to(torch.bfloat16)), offs, bool(pow2))[1]
    assert s[0, 11] == plain[0, 11] and s[2, 11] == plain[2, 11]  # ... and the other groups' scales do not move


def test_the_jagged_casts_of_the_fixture_are_the_recorded_bytes():
    G = fixture()
    for key, t in (("go_j", "go"), ("a_j", "a")):
        q_t, s, _ = ops.fp8_train_quantize_group_colwise_t(_bf16(G[t]).to(DEV), _dev(G["offs"]), True)
        np.testing.assert_array_equal(_u8(q_t).T, G[key + "_q"])
        np.testing.assert_array_equal(_u32(s).reshape(-1), _u32(G[key + "_s"]))


# ---- the 3-D transposing cast ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pow2", [0, 1])
def test_the_3d_cast_equals_the_2d_cast_of_every_expert(pow2):
    w = _bf16(_randn_bits((3, 144, 272), 21, 0.05)).to(DEV)
    q_t, s, inv = ops.fp8_train_quantize_colwise_t_3d(w, bool(pow2))
    assert tuple(q_t.shape) == (3, 272, 144) and tuple(s.shape) == tuple(inv.shape) == (3, 272) and q_t.is_contiguous()
    for e in range(3):
        q2, s2, inv2 = ops.fp8_train_quantize_colwise_t(w[e], bool(pow2))
        assert torch.equal(q_t[e].view(torch.uint8), q2.view(torch.uint8)), e
        assert torch.equal(s[e].view(torch.int32), s2.reshape(-1).view(torch.int32)) and torch.equal(inv[e].view(torch.int32), inv2.reshape(-1).view(torch.int32))


def test_the_3d_cast_of_the_fixture_is_the_recorded_transpose_rhs():
    G = fixture()
    q_t, s, _ = ops.fp8_train_quantize_colwise_t_3d(_bf16(G["w"]).to(DEV), True)
    np.testing.assert_array_equal(_u8(q_t), G["w3_q"])
    np.testing.assert_array_equal(_u32(s).reshape(G["w3_s"].shape), _u32(G["w3_s"]))


# ---- the weight-gradient GEMM through the C ABI ------------------------------------------------------------------------------------------
class _Slab:
    """One expert's [N, K] slab of a guarded [E * N, K] buffer, as tests/_parity.problems reads a buffer."""

    def __init__(self, buf, e, N):
        self.buf, self.lo, self.M, self.N, self.dtype, self.sentinel = buf, e * N, N, buf.N, buf.dtype, buf.sentinel
        self.out = buf.out[self.lo:self.lo + N]

    def bits(self):
        return self.buf.bits()[self.lo:self.lo + self.M]

    def guard_problems(self):
        return self.buf.guard_problems()


@functools.lru_cache(maxsize=None)
def _wgrad_operands(M, N, K):
    return _randn_bits((M, N), 31 + M, 0.01), _randn_bits((M, K), 32 + M)


class WRun:
    """The restatement's jagged casts of drawn grad_out [M, N] and x [M, K], the launch, and the float64 oracle per expert."""

    def __init__(self, offs, M, N, K):
        gb, xb = _wgrad_operands(M, N, K)
        self.M, self.N, self.K = M, N, K
        self.ends = [M] if offs is None else list(offs)
        self.E = len(self.ends)
        gq, gs, ginv = R.group_colwise(gb, self.ends)
        xq, xs, xinv = R.group_colwise(xb, self.ends)
        self.g, self.x = _dev(gq.T), _dev(xq.T)  # [N, M], [K, M]
        self.ginv, self.xinv = _dev(ginv), _dev(xinv)
        self.offs = None if offs is None else _dev(np.asarray(offs, dtype=np.int32))
        ref, mag = R.wgrad(gq, gs, xq, xs, self.ends, with_mag=True)
        self.ref, self.S = torch.from_numpy(ref).to(DEV), torch.from_numpy(mag).to(DEV)
        self.sizes = np.diff([0] + self.ends)

    def launch(self, buf):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _lib.check(_lib.lib().ao_fp8_grouped_mm_wgrad(p(self.g), p(self.ginv), p(self.x), p(self.xinv), p(self.offs), p(buf.out), self.M, self.N,
                                                      self.K, self.E, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()

    def run(self):
        buf = _parity.Guarded(self.E * self.N, self.K, torch.bfloat16, torch.device(DEV, 0))
        self.launch(buf)
        worst = 0.0
        for e, n in enumerate(self.sizes):
            slab = _Slab(buf, e, self.N)
            msgs = _parity.problems(slab, ref64=self.ref[e], S=self.S[e], K=int(n), k_floor=K_FLOOR_E4M3_MX, equal=EQUAL_GROUPED_MX)
            assert not msgs, "expert %d (%d tokens): " % (e, n) + "; ".join(msgs)
            worst = max(worst, _parity.k_needed(slab.out, self.ref[e], self.S[e], torch.bfloat16))
            if n == 0:
                assert not bool(slab.bits().any()), "an empty group's slab must be exactly zero"
        first = buf.bits().clone()
        buf.poison(_parity.SENTINEL2)
        self.launch(buf)
        assert not buf.guard_problems(), buf.guard_problems()
        assert torch.equal(buf.bits(), first), "the second launch gave other bits"
        return first, worst


WGRAD = [([48, 48, 208, 240], 256), ([128, 256], 256), ([0, 0, 16], 16)]


@pytest.mark.parametrize("offs,M", WGRAD, ids=["-".join(map(str, o)) for o, _ in WGRAD])
def test_wgrad_parity(offs, M):
    _, worst = WRun(offs, M, 144, 272).run()
    print("fp8 wgrad offs=%s M=%d N=144 K=272: the worst element needs max(K, k_floor) >= %.0f" % (offs, M, worst))


def test_wgrad_without_offs_is_one_group_of_every_token():
    one, _ = WRun([256], 256, 144, 272).run()
    none, _ = WRun(None, 256, 144, 272).run()
    assert torch.equal(one, none)


# ---- the Function ------------------------------------------------------------------------------------------------------------------------
def _fixture_operands(requires=(True, True)):
    G = fixture()
    a = _bf16(G["a"]).to(DEV).requires_grad_(requires[0])
    w = _bf16(G["w"]).to(DEV).requires_grad_(requires[1])
    return a, w, _bf16(G["go"]).to(DEV), _dev(G["offs"])


@functools.lru_cache(maxsize=None)
def _fixture_run():
    a, w, go, offs = _fixture_operands()
    out = _to_fp8_rowwise_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs, pad_token_groups_for_grouped_mm=False)
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach(), a.grad, w.grad


def test_the_function_is_the_ops_on_hand_made_casts():
    G = fixture()
    a, w, go, offs = _fixture_operands((False, False))
    out, grad_a, grad_w = _fixture_run()
    f8 = torch.float8_e4m3fn
    hand_out = ops.fp8_grouped_mm(_dev(G["a_r_q"], f8), _dev(1.0 / G["a_r_s"]), _dev(G["bt_c_q"].transpose(0, 2, 1), f8),
                                  _dev(1.0 / G["bt_c_s"].reshape(MAKER.E, MAKER.N)), offs)
    hand_ga = ops.fp8_grouped_mm(_dev(G["go_r_q"], f8), _dev(1.0 / G["go_r_s"]), _dev(G["w3_q"], f8),
                                 _dev(1.0 / G["w3_s"].reshape(MAKER.E, MAKER.K)), offs)
    hand_gw = ops.fp8_grouped_mm_wgrad(_dev(G["go_j_q"].T, f8), _dev(1.0 / G["go_j_s"].reshape(MAKER.E, MAKER.N)), _dev(G["a_j_q"].T, f8),
                                       _dev(1.0 / G["a_j_s"].reshape(MAKER.E, MAKER.K)), offs, MAKER.N, MAKER.K)
    assert torch.equal(out.view(torch.int16), hand_out.view(torch.int16))
    assert torch.equal(grad_a.view(torch.int16), hand_ga.view(torch.int16))
    assert torch.equal(grad_w.view(torch.int16), hand_gw.view(torch.int16))
    assert out.dtype == grad_a.dtype == grad_w.dtype == torch.bfloat16 and tuple(grad_w.shape) == (MAKER.E, MAKER.N, MAKER.K)
    again = torch.ops.ao_mi355.fp8_grouped_mm_wgrad(_dev(G["go_j_q"].T, f8), _dev(1.0 / G["go_j_s"].reshape(MAKER.E, MAKER.N)), _dev(G["a_j_q"].T, f8),
                                                    _dev(1.0 / G["a_j_s"].reshape(MAKER.E, MAKER.K)), offs, MAKER.N, MAKER.K)
    assert torch.equal(again.view(torch.int16), hand_gw.view(torch.int16))


def _mags():
    G = fixture()
    E, N, K, offs = MAKER.E, MAKER.N, MAKER.K, G["offs"]
    ab = lambda q, s: np.abs(R.T.dequant(q, s))  # noqa: E731
    mag_o, mag_a = np.zeros((MAKER.M, N)), np.zeros((MAKER.M, K))
    lo = 0
    for e, hi in enumerate(int(o) for o in offs):
        mag_o[lo:hi] = ab(G["a_r_q"][lo:hi], G["a_r_s"][lo:hi]) @ ab(G["bt_c_q"][e], G["bt_c_s"][e])
        mag_a[lo:hi] = ab(G["go_r_q"][lo:hi], G["go_r_s"][lo:hi]) @ ab(G["w3_q"][e], G["w3_s"][e].reshape(K, 1)).T
        lo = hi
    mag_w = R.wgrad(G["go_j_q"], G["go_j_s"].reshape(E, N), G["a_j_q"], G["a_j_s"].reshape(E, K), offs, with_mag=True)[1]
    return mag_o, mag_a, mag_w


def _within(y_bits, ref_bits, mag):
    y, ref = _f32(y_bits).astype(np.float64), _f32(ref_bits).astype(np.float64)
    return np.all(np.abs(y - ref) <= np.abs(ref) * 2.0 ** -7 + mag.reshape(ref.shape) * 2.0 ** -16)


def test_the_function_stays_within_the_bound_of_the_fixture():
    G = fixture()
    out, grad_a, grad_w = _fixture_run()
    mag_o, mag_a, mag_w = _mags()
    for name, y, mag in (("out", out, mag_o), ("grad_a", grad_a, mag_a), ("grad_w", grad_w, mag_w)):
        same = np.mean(_bits(y) == G[name])
        print("%s: %.4f of the elements have the recording's bits" % (name, same))
        assert _within(_bits(y), G[name], mag), name


def _sqnr(y, ref):
    return 10 * np.log10(np.sum(ref.astype(np.float64) ** 2) / np.sum((y.astype(np.float64) - ref) ** 2))


def _fp32_reference(a, w, go, offs):
    """Per-group fp32 matmuls on the CPU: out [M, N], grad_A [M, K], grad_W [E, N, K]."""
    a, w, go = a.detach().float().cpu().numpy(), w.detach().float().cpu().numpy(), go.float().cpu().numpy()
    y, ga, gw = np.zeros((a.shape[0], w.shape[1]), np.float32), np.zeros_like(a), np.zeros_like(w)
    lo = 0
    for e, hi in enumerate(int(o) for o in offs):
        y[lo:hi], ga[lo:hi], gw[e] = a[lo:hi] @ w[e].T, go[lo:hi] @ w[e], go[lo:hi].T @ a[lo:hi]
        lo = hi
    return y, ga, gw


def _meets_the_bars(got, want, label):
    vals = [_sqnr(g.float().cpu().numpy(), r) for g, r in zip(got, want)]
    print("%s SQNR vs fp32 matmuls: out %.2f dB, grad_A %.2f dB, grad_B %.2f dB" % (label, *vals))
    assert vals[0] >= 18.0 and vals[1] >= 17.0 and vals[2] >= 17.0, vals


def test_sqnr_against_fp32_matmuls_meets_the_references_bars():
    """test/float8/test_base.py:313-319: >= 18 dB on the output, >= 17 dB on the gradients."""
    a, w, go, offs = _fixture_operands((False, False))
    _meets_the_bars(_fixture_run(), _fp32_reference(a, w, go, fixture()["offs"]), "fixture")


@pytest.mark.parametrize("frozen", ["A", "B_t"])
def test_a_frozen_operand_skips_its_casts_and_its_gemm(frozen, monkeypatch):
    calls = []
    for name in ("fp8_train_quantize_rowwise", "fp8_train_quantize_colwise_t_3d", "fp8_train_quantize_group_colwise_t", "fp8_grouped_mm",
                 "fp8_grouped_mm_wgrad"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *args, _real=real, _name=name, **kw: (calls.append(_name), _real(*args, **kw))[1])
    a, w, go, offs = _fixture_operands((frozen != "A", frozen != "B_t"))
    out = _to_fp8_rowwise_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs, pad_token_groups_for_grouped_mm=False)
    forward = list(calls)
    assert forward == ["fp8_train_quantize_rowwise", "fp8_train_quantize_rowwise", "fp8_grouped_mm"]
    out.backward(go)
    backward = calls[len(forward):]
    full = _fixture_run()
    if frozen == "A":
        assert backward == ["fp8_train_quantize_group_colwise_t", "fp8_train_quantize_group_colwise_t", "fp8_grouped_mm_wgrad"]
        assert a.grad is None and torch.equal(w.grad.view(torch.int16), full[2].view(torch.int16))
    else:
        assert backward == ["fp8_train_quantize_rowwise", "fp8_train_quantize_colwise_t_3d", "fp8_grouped_mm"]
        assert w.grad is None and torch.equal(a.grad.view(torch.int16), full[1].view(torch.int16))


def test_a_non_contiguous_grad_out_works():
    a, w, go, offs = _fixture_operands()
    out = _to_fp8_rowwise_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs, pad_token_groups_for_grouped_mm=False)
    strided = go.t().contiguous().t()
    assert not strided.is_contiguous()
    out.backward(strided)
    full = _fixture_run()
    assert torch.equal(a.grad.view(torch.int16), full[1].view(torch.int16)) and torch.equal(w.grad.view(torch.int16), full[2].view(torch.int16))


def test_padding_equals_the_unpadded_function_on_the_padded_tensors():
    G = fixture()
    offs_np = np.array([40, 200, 250], dtype=np.int32)
    offs = _dev(offs_np)
    a0, go = _bf16(G["a"][:250]).to(DEV), _bf16(G["go"][:250]).to(DEV)
    a = a0.clone().requires_grad_(True)
    w = _bf16(G["w"]).to(DEV).requires_grad_(True)
    out = _to_fp8_rowwise_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs)  # the default: padding on
    out.backward(go)
    assert tuple(out.shape) == (250, MAKER.N) and tuple(a.grad.shape) == (250, MAKER.K)
    # by hand: pad, run without padding, cut the pad rows out again
    a_pad, starts, ends = pad_token_groups(a0, offs, 16)
    go_pad, _, _ = pad_token_groups(go, offs, 16)
    ends_np, starts_np = ends.cpu().numpy(), starts.cpu().numpy()
    assert a_pad.shape[0] % 16 == 0 and not (ends_np % 16).any() and list(ends_np - starts_np) == [48, 160, 64]
    a2 = a_pad.clone().requires_grad_(True)
    w2 = _bf16(G["w"]).to(DEV).requires_grad_(True)
    out2 = _to_fp8_rowwise_then_scaled_grouped_mm(a2, w2.transpose(-2, -1), ends, pad_token_groups_for_grouped_mm=False)
    out2.backward(go_pad)
    rows = torch.cat([torch.arange(int(s), int(s) + n) for s, n in zip(starts_np, np.diff([0] + list(offs_np)))]).to(DEV)
    assert torch.equal(out.view(torch.int16), out2[rows].view(torch.int16))
    assert torch.equal(a.grad.view(torch.int16), a2.grad[rows].view(torch.int16))
    assert torch.equal(w.grad.view(torch.int16), w2.grad.view(torch.int16))
    _meets_the_bars((out.detach(), a.grad, w.grad), _fp32_reference(a0, w, go, offs_np), "padded [40, 200, 250]")


class ToyExperts(nn.Module):
    def __init__(self, w, lin_w):
        super().__init__()
        self.w = nn.Parameter(w.clone())
        self.lin = nn.Linear(lin_w.shape[1], lin_w.shape[0], bias=False, device=DEV, dtype=torch.bfloat16)
        self.lin.weight.data.copy_(lin_w)

    def forward(self, x, offs):
        return self.lin(torch._grouped_mm(x, self.w.transpose(-2, -1), offs=offs))


def _converted_and_direct():
    from ao_amd.float8.float8_linear import matmul_with_hp_or_float8_args
    a, w, go, offs = _fixture_operands((True, False))
    lin_w = _bf16(_randn_bits((144, 128), 41, 0.05)).to(DEV)
    go2 = _bf16(_randn_bits((256, 144), 42, 0.01)).to(DEV)
    cfg = Float8TrainingOpConfig()
    model = ToyExperts(w, lin_w)
    quantize_(model, cfg, filter_fn=lambda mod, fqn: isinstance(mod, (ToyExperts, nn.Linear)))
    assert type(model.w.data) is FG.Float8TrainingWeightWrapperTensor and type(model.lin.weight.data) is FG.Float8TrainingWeightWrapperTensor
    y = model(a, offs)
    y.backward(go2)
    got = (y.detach(), a.grad, model.w.grad, model.lin.weight.grad)
    a2 = a.detach().clone().requires_grad_(True)
    w2, l2 = w.detach().clone().requires_grad_(True), lin_w.clone().requires_grad_(True)
    h = _to_fp8_rowwise_then_scaled_grouped_mm(a2, w2.transpose(-2, -1), offs, pad_token_groups_for_grouped_mm=False)
    y2 = matmul_with_hp_or_float8_args.apply(h, l2.t(), cfg._linear_mm_config, cfg._float8_linear_config)
    y2.backward(go2)
    return got, (y2.detach(), a2.grad, w2.grad, l2.grad)


def test_quantize_converted_experts_run_forward_and_backward_with_the_direct_calls_bits():
    got, want = _converted_and_direct()
    for name, g, r in zip(("out", "grad_x", "grad_w", "grad_lin"), got, want):
        assert g is not None and g.shape == r.shape and torch.equal(g.contiguous().view(torch.int16), r.contiguous().view(torch.int16)), name


def test_the_casts_and_the_wgrad_can_be_captured_in_a_graph():
    G = fixture()
    a, w, go, offs = _fixture_operands((False, False))

    def step():
        g_t, _, g_inv = ops.fp8_train_quantize_group_colwise_t(go, offs, True)
        x_t, _, x_inv = ops.fp8_train_quantize_group_colwise_t(a, offs, True)
        w_t, w_s, _ = ops.fp8_train_quantize_colwise_t_3d(w, True)
        return g_t, x_t, w_t, w_s, ops.fp8_grouped_mm_wgrad(g_t, g_inv, x_t, x_inv, offs, MAKER.N, MAKER.K)

    eager = [t.clone() for t in step()]  # warm: the allocator's pools, the kernel's LDS attribute
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            captured = step()
        for t in captured:
            t.zero_()
        graph.replay()
    torch.cuda.synchronize()
    for e, c in zip(eager, captured):
        assert torch.equal(e.view(torch.uint8), c.view(torch.uint8))
    np.testing.assert_array_equal(_u8(captured[0]).T, G["go_j_q"])
