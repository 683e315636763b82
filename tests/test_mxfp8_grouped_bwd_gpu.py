"""GPU: the backward of the MXFP8 MoE grouped GEMM -- mx_wgrad_kernel through the C ABI against a float64 reference, and the autograd
Function of _to_mxfp8_then_scaled_grouped_mm against the fixture written from the reference (tests/golden/mxfp8_grouped_bwd.npz).

The C ABI cases write into guarded, poisoned [E * N, K] buffers (tests/_parity.py), launch twice into differently poisoned buffers and
must give the same bits.  Operands as in test_route_parity_grouped_gpu.py: every finite e4m3 code, E8M0 scales 127 + U{-12..12} per
(32-token block, row).  Every expert's [N, K] slab is checked with K = that expert's token count, the scaled MFMA's floor on K
(test_route_parity_gpu.K_FLOOR_E4M3_MX = 1408) and the grouped MX equal fraction (0.96).
Measured on these cases on an MI355X (every case prints its own): the worst element needs max(K, floor) >= 1374, on ([128, 128], 256,
256, 384); 632, 805 and 825 on the three cases with masked steps (profiles/pytest_gpu_mxfp8_bwd.log).
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import _parity
from ao_amd import _lib, ops
from ao_amd.prototype import mx
from oracle import mx_ref
from test_route_parity_grouped_gpu import EQUAL_GROUPED_MX
from test_route_parity_gpu import K_FLOOR_E4M3_MX, Draw, _e4m3

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"


class _Slab:
    """One expert's [N, K] slab of a guarded [E * N, K] buffer, as tests/_parity.problems reads a buffer."""

    def __init__(self, buf, e, N):
        self.buf, self.lo, self.M, self.N, self.dtype, self.sentinel = buf, e * N, N, buf.N, buf.dtype, buf.sentinel
        self.out = buf.out[self.lo:self.lo + N]

    def bits(self):
        return self.buf.bits()[self.lo:self.lo + self.M]

    def guard_problems(self):
        return self.buf.guard_problems()


class WRun:
    """Operands of a wgrad case in the layout ao_mxfp8_quantize_colwise writes, the launch, and the float64 reference per expert."""

    def __init__(self, sizes, M, N, K, seed, exact=False):
        d = Draw(seed, torch.device(DEV, 0))
        self.sizes, self.M, self.N, self.K, self.E = sizes, M, N, K, len(sizes)
        self.offs = torch.tensor(np.cumsum(sizes), dtype=torch.int32, device=DEV)
        if exact:  # codes of 0, +-1, +-2, +-4 and scales 2^-2 .. 2^2: every partial sum is a small multiple of 2^-4
            table = torch.tensor([0x00, 0x38, 0x40, 0x48, 0xB8, 0xC0, 0xC8], dtype=torch.uint8, device=DEV)
            draw = lambda r: table[torch.randint(0, 7, (r, M), generator=d.g, device=DEV)]  # noqa: E731
            scale = lambda r: (125 + torch.randint(0, 5, (M // 32, r), generator=d.g, device=DEV)).to(torch.uint8)  # noqa: E731
            self.g, self.gs, self.x, self.xs = draw(N), scale(N), draw(K), scale(K)
        else:
            self.g, self.gs = d.fp8(N, M), d.e8m0(M // 32, N)
            self.x, self.xs = d.fp8(K, M), d.e8m0(M // 32, K)
        G = _e4m3(self.g) * torch.exp2(self.gs.double() - 127).t().repeat_interleave(32, 1)  # [N, M]
        X = _e4m3(self.x) * torch.exp2(self.xs.double() - 127).t().repeat_interleave(32, 1)  # [K, M]
        self.ref, self.S, lo = [], [], 0
        for n in sizes:
            self.ref.append(G[:, lo:lo + n] @ X[:, lo:lo + n].t())
            self.S.append(G[:, lo:lo + n].abs() @ X[:, lo:lo + n].abs().t())
            lo += n

    def buffer(self):
        return _parity.Guarded(self.E * self.N, self.K, torch.bfloat16, torch.device(DEV, 0))

    def launch(self, buf):
        p = lambda t: t.data_ptr()  # noqa: E731
        _lib.check(_lib.lib().ao_mxfp8_grouped_mm_wgrad(p(self.g), p(self.gs), p(self.x), p(self.xs), p(self.offs), p(buf.out), self.M, self.N, self.K,
                                                        self.E, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()

    def check(self, buf, exact=False):
        worst = 0.0
        for e, n in enumerate(self.sizes):
            slab = _Slab(buf, e, self.N)
            if exact:
                kw = dict(ref_bits=_parity.oracle_round(self.ref[e], torch.bfloat16).view(torch.int16))
            else:
                kw = dict(ref64=self.ref[e], S=self.S[e], K=n, k_floor=K_FLOOR_E4M3_MX, equal=EQUAL_GROUPED_MX)
                worst = max(worst, _parity.k_needed(slab.out, self.ref[e], self.S[e], torch.bfloat16))
            msgs = _parity.problems(slab, **kw)
            assert not msgs, "expert %d (%d tokens): " % (e, n) + "; ".join(msgs)
        return worst


CASES = [
    ([40, 0, 88, 0], 128, 144, 208),  # partial tiles both ways, a boundary inside a 32-block, empty groups in the middle and last, one k step
    ([1, 130, 125], 256, 128, 128),   # a one-token group, boundaries off every grid, groups spanning k steps that they share
    ([128, 128], 256, 256, 384),      # several tiles, no masks
    ([32, 31], 96, 128, 128),         # tokens past offs[-1] must not contribute
    ([0, 0], 32, 128, 128),           # all zeros
]


@pytest.mark.gpu
@pytest.mark.parametrize("sizes,M,N,K", CASES, ids=["%s:%d,%d,%d" % ("-".join(map(str, c[0])), *c[1:]) for c in CASES])
def test_wgrad_parity(sizes, M, N, K):
    run = WRun(sizes, M, N, K, 4000 + M + N + K)
    buf = run.buffer()
    run.launch(buf)
    worst = run.check(buf)
    print("wgrad %s M=%d N=%d K=%d: the worst element needs max(K, k_floor) >= %.0f" % (sizes, M, N, K, worst))
    if sum(sizes) == 0:
        assert not bool(buf.bits().any()), "no tokens: the output must be all zero"
    first = buf.bits().clone()
    buf.poison(_parity.SENTINEL2)
    run.launch(buf)
    assert not buf.guard_problems(), buf.guard_problems()
    assert torch.equal(buf.bits(), first), "the second launch gave other bits"


@pytest.mark.gpu
def test_wgrad_exact_sums():
    """Small integer codes and scales near 1: every fp32 partial sum is exact, so the output is the float64 sum rounded once."""
    run = WRun([40, 0, 88], 128, 128, 256, 4100, exact=True)
    buf = run.buffer()
    run.launch(buf)
    run.check(buf, exact=True)
    assert bool(buf.out[:128].any()) and not bool(buf.bits()[128:256].any())


@pytest.mark.gpu
def test_wgrad_of_no_tokens_zeroes_the_output():
    buf = _parity.Guarded(2 * 128, 128, torch.bfloat16, torch.device(DEV, 0))
    offs = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().ao_mxfp8_grouped_mm_wgrad(None, None, None, None, offs.data_ptr(), buf.out.data_ptr(), 0, 128, 128, 2,
                                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert not buf.guard_problems() and not bool(buf.bits().any())


# ---- the autograd Function against the reference's fixture -------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_mxfp8_bwd", os.path.join(HERE, "golden", "make_golden_mxfp8_bwd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bf16(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f32(bits):
    return _bf16(bits).float().numpy()


@functools.lru_cache(maxsize=None)
def fixture():
    return _generator().load()


def grads(pad=False, hp=False, contiguous_b_t=False):
    """(out, grad_A, grad_W [E, N, K]) of one forward + backward on the fixture's tensors, computed once per variant."""
    return _grads(bool(pad), bool(hp), bool(contiguous_b_t))


@functools.lru_cache(maxsize=None)
def _grads(pad, hp, contiguous_b_t):
    G = fixture()
    a = _bf16(G["a"]).to(DEV).requires_grad_(True)
    w = _bf16(G["w"]).to(DEV)
    if contiguous_b_t:
        b_t = w.transpose(-2, -1).contiguous().requires_grad_(True)
    else:
        w.requires_grad_(True)
        b_t = w.transpose(-2, -1)
    offs = torch.from_numpy(G["offs"]).to(DEV)
    y = mx._to_mxfp8_then_scaled_grouped_mm(a, b_t, offs, wgrad_with_hp=hp, pad_token_groups_for_grouped_mm=pad)
    y.backward(_bf16(G["go"]).to(DEV))
    gw = b_t.grad.transpose(-2, -1) if contiguous_b_t else w.grad
    assert a.grad.dtype == gw.dtype == y.dtype == torch.bfloat16
    return y.detach(), a.grad, gw


def _mags():
    """The oracle's sum |dq| |dq| behind every element of grad_input [M, K] and grad_weight [E, N, K], and the rowwise cast of grad_out."""
    G = fixture()
    go_q, go_s = mx_ref.to_mx(_f32(G["go"]), mx_ref.RCEIL)
    w_q = np.ascontiguousarray(G["w_n_q"].transpose(0, 2, 1))  # [E, K, N], blocks along N
    w_s = np.ascontiguousarray(G["w_n_s"].transpose(0, 2, 1))  # [E, K, N/32]
    _, mag_i = mx_ref.grouped_mm(go_q, go_s, w_q, w_s, G["offs"], return_abs=True)
    g = np.abs(mx_ref.mx_dequant_bf16(G["go_t_q"], G["go_t_s"]).astype(np.float64))  # [N, M]
    x = np.abs(mx_ref.mx_dequant_bf16(G["a_t_q"], G["a_t_s"]).astype(np.float64))    # [K, M]
    mag_w, lo = np.zeros(G["w"].shape), 0
    for e, hi in enumerate(G["offs"]):
        mag_w[e] = g[:, lo:hi] @ x[:, lo:hi].T
        lo = int(hi)
    return (go_q, go_s, w_q, w_s), mag_i, mag_w


def _within(y_bits, ref_bits, mag):
    y, ref = _f32(y_bits).astype(np.float64), _f32(ref_bits).astype(np.float64)
    return np.all(np.abs(y - ref) <= np.abs(ref) * 2.0 ** -7 + mag * 2.0 ** -16)


def _sqnr(y, ref):
    return 10 * np.log10(np.sum(ref.astype(np.float64) ** 2) / np.sum((y.astype(np.float64) - ref) ** 2))


@pytest.mark.gpu
def test_the_backwards_casts_equal_the_fixture():
    G = fixture()
    for name, src in (("go_t", "go"), ("a_t", "a")):
        q, s = ops.mxfp8_quantize_colwise(_bf16(G[src]).to(DEV))
        np.testing.assert_array_equal(q.t().contiguous().view(torch.uint8).cpu().numpy(), G[name + "_q"])
        np.testing.assert_array_equal(s.contiguous().view(torch.uint8).cpu().numpy(), G[name + "_s"])
    q, s = ops.mxfp8_quantize_3d(_bf16(G["w"]).to(DEV))
    np.testing.assert_array_equal(q.contiguous().view(torch.uint8).cpu().numpy(), G["w_n_q"])
    np.testing.assert_array_equal(s.transpose(-2, -1).contiguous().view(torch.uint8).cpu().numpy(), G["w_n_s"])
    # a contiguous [E, K, N] B_t is cast rowwise along N: the same codes and scales
    q, s = ops.mxfp8_quantize(_bf16(G["w"]).to(DEV).transpose(-2, -1).contiguous())
    np.testing.assert_array_equal(q.transpose(-2, -1).contiguous().view(torch.uint8).cpu().numpy(), G["w_n_q"])
    np.testing.assert_array_equal(s.transpose(-2, -1).contiguous().view(torch.uint8).cpu().numpy(), G["w_n_s"])


@pytest.mark.gpu
def test_grad_input_is_the_forward_gemm_on_the_casts_along_n():
    G = fixture()
    (go_q, go_s, w_q, w_s), _, _ = _mags()
    t = lambda v: torch.from_numpy(v).to(DEV)  # noqa: E731
    hand = ops.mxfp8_grouped_mm(t(go_q), t(go_s), t(w_q), t(w_s), t(G["offs"]))
    np.testing.assert_array_equal(_bits(grads()[1]), _bits(hand))
    np.testing.assert_array_equal(_bits(grads(contiguous_b_t=True)[1]), _bits(hand))


@pytest.mark.gpu
def test_grad_weight_is_the_wgrad_op_on_the_colwise_casts():
    G = fixture()
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)  # noqa: E731
    E, N, K = G["w"].shape
    hand = ops.mxfp8_grouped_mm_wgrad(t(G["go_t_q"]), t(G["go_t_s"].T), t(G["a_t_q"]), t(G["a_t_s"].T), t(G["offs"]), N, K)
    assert tuple(hand.shape) == (E, N, K)
    np.testing.assert_array_equal(_bits(grads()[2]), _bits(hand))
    np.testing.assert_array_equal(_bits(grads(contiguous_b_t=True)[2]), _bits(hand))
    # the strided views that the colwise cast returns, through the dispatcher
    import ao_amd.torch_ops  # noqa: F401

    g_t, g_ts = ops.mxfp8_quantize_colwise(_bf16(G["go"]).to(DEV))
    x_t, x_ts = ops.mxfp8_quantize_colwise(_bf16(G["a"]).to(DEV))
    assert not g_t.is_contiguous() and not g_ts.is_contiguous()
    again = torch.ops.ao_mi355.mxfp8_grouped_mm_wgrad(g_t, g_ts, x_t, x_ts, t(G["offs"]), N, K)
    np.testing.assert_array_equal(_bits(again), _bits(hand))


@pytest.mark.gpu
def test_wgrad_with_hp_is_the_bf16_grouped_mm():
    G = fixture()
    go, a, offs = _bf16(G["go"]).to(DEV), _bf16(G["a"]).to(DEV), torch.from_numpy(G["offs"]).to(DEV)
    want = torch._grouped_mm(go.transpose(-2, -1), a, offs=offs, out_dtype=torch.bfloat16)
    _, gi, gw = grads(hp=True)
    np.testing.assert_array_equal(_bits(gw), _bits(want))
    np.testing.assert_array_equal(_bits(gi), _bits(grads()[1]))  # the grad_input does not depend on it


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
@pytest.mark.parametrize("hp", [False, True], ids=["mx", "hp"])
def test_gradients_stay_within_the_forward_bound_of_the_fixture(pad, hp):
    G = fixture()
    tag = "%s_%s" % ("pad" if pad else "nopad", "hp" if hp else "mx")
    _, mag_i, mag_w = _mags()
    y, gi, gw = grads(pad=pad, hp=hp)
    assert tuple(y.shape) == G["out"].shape and tuple(gi.shape) == G["a"].shape and tuple(gw.shape) == G["w"].shape
    assert not bool(gw[1].any()), "the empty expert's slab must be zero"
    assert _within(_bits(gi), G["gi_" + tag], mag_i)
    assert _within(_bits(gw), G["gw_" + tag], mag_w)


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
def test_sqnr_against_fp32_matmuls_meets_the_references_bars(pad):
    """test_mxfp8_grouped_mm.py:318-340: >= 27 dB on the output, 25 dB on the input gradient, 24 dB on the weight gradient."""
    G = fixture()
    a, w, go = _f32(G["a"]), _f32(G["w"]), _f32(G["go"])
    out, gi, gw, lo = np.zeros(G["out"].shape, np.float32), np.zeros(a.shape, np.float32), np.zeros(w.shape, np.float32), 0
    for e, hi in enumerate(G["offs"]):
        out[lo:hi] = a[lo:hi] @ w[e].T
        gi[lo:hi] = go[lo:hi] @ w[e]
        gw[e] = go[lo:hi].T @ a[lo:hi]
        lo = int(hi)
    y, ga, gwt = grads(pad=pad)
    got = [_sqnr(_f32(_bits(t)), r) for t, r in ((y, out), (ga, gi), (gwt, gw))]
    print("SQNR vs fp32: out %.2f dB, grad_input %.2f dB, grad_weight %.2f dB" % tuple(got))
    assert got[0] >= 27.0 and got[1] >= 25.0 and got[2] >= 24.0


@pytest.mark.gpu
def test_calls_without_grad_keep_their_path_and_bits():
    G = fixture()
    a, w, offs = _bf16(G["a"]).to(DEV), _bf16(G["w"]).to(DEV), torch.from_numpy(G["offs"]).to(DEV)
    plain = mx._to_mxfp8_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs)
    assert not plain.requires_grad and plain.grad_fn is None
    ag, wg = a.clone().requires_grad_(True), w.clone().requires_grad_(True)
    with torch.no_grad():
        quiet = mx._to_mxfp8_then_scaled_grouped_mm(ag, wg.transpose(-2, -1), offs, wgrad_with_hp=True, pad_token_groups_for_grouped_mm=True)
    assert not quiet.requires_grad
    np.testing.assert_array_equal(_bits(plain), _bits(quiet))
    np.testing.assert_array_equal(_bits(plain), _bits(grads()[0]))  # and the Function's forward is that call
    assert _within(_bits(plain), G["out"], mx_ref.grouped_mm(*_forward_casts(), G["offs"], return_abs=True)[1])


def _forward_casts():
    G = fixture()
    a_q, a_s = mx_ref.to_mx(_f32(G["a"]), mx_ref.RCEIL)
    w_q, w_s = mx_ref.to_mx(_f32(G["w"]), mx_ref.RCEIL)
    return a_q, a_s, w_q, w_s
