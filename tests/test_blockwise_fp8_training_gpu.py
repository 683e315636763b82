"""GPU: blockwise float8 training -- the HIP block-local casts against the numpy restatement (tests/blockwise_fp8_training_ref.py, itself
pinned to the fixture written from the reference's torch functions), byte for byte; the weight-gradient GEMM against the fp32 chain on
exact sums and against float64 on Gaussian operands; the autograd Function against ops.fp8_block_mm / ops.fp8_block_mm_wgrad on hand-made
casts (bit-equal); frozen operands, no_grad, quantize_, the reference's SQNR bars and graph capture.

K_FLOOR and EQUAL are the project's constants for this instruction (tests/test_fp8_block_gpu.py): conditions, not targets.  Every
Gaussian case and both SQNR cases print their figures before they assert (profiles/pytest_gpu_fp8_block_training.log).
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
from torch import nn

import _parity
import blockwise_fp8_training_ref as R
from ao_amd import _lib, ops
from ao_amd.prototype.blockwise_fp8_training import Float8BlockwiseLinear, Float8BlockwiseLinearConfig, fp8_blockwise_mm
from ao_amd.quantization import quantize_

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
# Measured on an MI355X over the four Gaussian cases (profiles/pytest_gpu_fp8_block_training.log): worst k_needed 523 at (128, 128, 128),
# at most 247 elsewhere; lowest equal fraction 0.9675 at (384, 128, 256).  Both caps are far from binding.
K_FLOOR = 896
EQUAL = 0.95
WGRAD_SHAPES = [(128, 128, 128), (384, 128, 256), (256, 384, 128), (640, 256, 256)]  # (M, N, K); 640: five token steps over two stages


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    return _load("make_golden_blockwise_fp8_training").load()


def _bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _u8(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _u32(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t, dtype=np.float32)).view(np.uint32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the casts -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cast_input(name):
    """bf16 bits [R, C]: a fixture tensor by name, or a seeded matrix whose rows span 2^-12 .. 2^12."""
    if isinstance(name, str):
        xb = fixture()[name]
        return xb.reshape(-1, xb.shape[-1])
    g = torch.Generator().manual_seed(1000 + name[0] + name[1])
    x = torch.randn(*name, generator=g) * torch.exp2(torch.randint(-12, 13, (name[0], 1), generator=g).float())
    return x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def ref_rows(name):
    return R.cast_rows(cast_input(name))[:2]


@functools.lru_cache(maxsize=None)
def ref_cols(name):
    return R.cast_cols(cast_input(name))[:2]


@functools.lru_cache(maxsize=None)
def ref_weight(name):
    return R.cast_weight(cast_input(name))[:2]


def _same(got, want):
    q, inv = got
    wq, winv = want
    assert q.dtype == torch.float8_e4m3fn and inv.dtype == torch.float32 and tuple(q.shape) == wq.shape and tuple(inv.shape) == winv.shape
    np.testing.assert_array_equal(_u8(q), wq)
    np.testing.assert_array_equal(_u32(inv), _u32(winv))


ROW_ONLY = [(1, 128), (5, 384), (130, 256)]
BOTH = [(128, 128), (256, 384), (384, 128), "x", "go", "edge"]
WEIGHTS = [(128, 128), (256, 384), (384, 128), "w", "edge"]
_id = lambda s: s if isinstance(s, str) else "%dx%d" % s  # noqa: E731


@pytest.mark.parametrize("name", ROW_ONLY + BOTH, ids=_id)
def test_the_row_cast_equals_the_restatement(name):
    x = _bf16(cast_input(name)).to(DEV)
    rows, cols = ops.fp8_block_train_cast(x)
    assert cols is None
    _same(rows, ref_rows(name))


@pytest.mark.parametrize("name", BOTH, ids=_id)
def test_the_column_cast_and_the_one_read_form_equal_the_restatement(name):
    x = _bf16(cast_input(name)).to(DEV)
    rows, cols = ops.fp8_block_train_cast(x, rows=False, cols=True)
    assert rows is None
    _same(cols, ref_cols(name))
    rows, cols = ops.fp8_block_train_cast(x, rows=True, cols=True)  # both directions in one read: the bytes of the two calls
    _same(rows, ref_rows(name))
    _same(cols, ref_cols(name))


def test_the_casts_equal_the_fixture():
    """The operands of the three GEMMs, taken through the ops as the Function takes them, are the reference's recorded bytes."""
    G = fixture()
    for t in ("x", "go", "edge"):
        rows, cols = ops.fp8_block_train_cast(_bf16(cast_input(t)).to(DEV), rows=True, cols=True)
        np.testing.assert_array_equal(_u8(rows[0]), G[t + "_row_q"])
        np.testing.assert_array_equal(_u32(rows[1]), _u32(G[t + "_row_inv"]))
        np.testing.assert_array_equal(_u8(cols[0].t()), G[t + "_col_q"])
        np.testing.assert_array_equal(_u32(cols[1]), _u32(G[t + "_col_inv"]))
    for t in ("w", "edge"):
        q, inv = ops.fp8_block_train_cast_weight(_bf16(cast_input(t)).to(DEV))
        np.testing.assert_array_equal(_u8(q), G[t + "_blk_q"])
        np.testing.assert_array_equal(_u32(inv), _u32(G[t + "_blk_inv"]))


@pytest.mark.parametrize("name", WEIGHTS, ids=_id)
def test_the_weight_cast_equals_the_restatement_in_either_layout(name):
    w = _bf16(cast_input(name)).to(DEV)
    want = ref_weight(name)
    plain = ops.fp8_block_train_cast_weight(w)
    trans = ops.fp8_block_train_cast_weight(w, transposed=True)
    both = ops.fp8_block_train_cast_weight(w, transposed=None)
    _same(plain, want)
    _same(both[0], want)
    for q_t, inv_t in (trans, both[1]):  # q_t == q.T and inv_t == inv.T
        assert q_t.is_contiguous() and inv_t.is_contiguous()
        _same((q_t, inv_t), (np.ascontiguousarray(want[0].T), np.ascontiguousarray(want[1].T)))
    # and the transposed layout is the plain cast of w.t(): a block's codes do not depend on the layout
    _same(ops.fp8_block_train_cast_weight(w.t().contiguous()), (np.ascontiguousarray(want[0].T), np.ascontiguousarray(want[1].T)))


def test_odd_row_counts_cast_along_rows_only_and_empty_inputs_launch_nothing():
    x = _bf16(cast_input((130, 256))).to(DEV)
    with pytest.raises(ValueError, match="130 rows"):
        ops.fp8_block_train_cast(x, rows=True, cols=True)
    (q, inv), _ = ops.fp8_block_train_cast(x[:0])
    assert tuple(q.shape) == (0, 256) and tuple(inv.shape) == (0, 2)
    _, (qt, invt) = ops.fp8_block_train_cast(x[:0], rows=False, cols=True)
    assert tuple(qt.shape) == (256, 0) and tuple(invt.shape) == (0, 256)
    out = ops.fp8_block_mm_wgrad(qt[:128], invt[:, :128], qt, invt)  # M == 0: zeros
    assert tuple(out.shape) == (128, 256) and not bool(out.any())


@pytest.mark.parametrize("name", ["edge", (130, 256)], ids=_id)
def test_the_c_entry_points_stay_inside_their_outputs(name):
    """Guarded, poisoned buffers: every cast entry writes exactly its outputs and nothing outside; the one-read form writes the bytes of
    the single-direction calls."""
    xb = cast_input(name)
    R_, C = xb.shape
    cols = R_ % 128 == 0
    x = _bf16(xb).to(DEV)
    dev = torch.device(DEV, 0)
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    F = lambda n: _parity.Guarded(1, n, torch.float32, dev)  # noqa: E731
    B = lambda n: _parity.Guarded(1, n // 2, torch.bfloat16, dev)  # noqa: E731  (n bytes)
    by = lambda b: b.bits().contiguous().view(torch.uint8).reshape(-1).cpu().numpy()  # noqa: E731
    p = lambda b: b.out.data_ptr()  # noqa: E731
    q, inv = B(R_ * C), F(R_ * C // 128)
    _lib.check(lib.ao_fp8_block_train_cast(x.data_ptr(), p(q), p(inv), None, None, R_, C, st))
    bufs = [q, inv]
    if cols:
        qt, invt, q2, inv2, qt2, invt2 = B(R_ * C), F(R_ // 128 * C), B(R_ * C), F(R_ * C // 128), B(R_ * C), F(R_ // 128 * C)
        _lib.check(lib.ao_fp8_block_train_cast(x.data_ptr(), None, None, p(qt), p(invt), R_, C, st))
        _lib.check(lib.ao_fp8_block_train_cast(x.data_ptr(), p(q2), p(inv2), p(qt2), p(invt2), R_, C, st))
        wq, winv, wqt, winvt = B(R_ * C), F(R_ * C // 16384), B(R_ * C), F(R_ * C // 16384)
        _lib.check(lib.ao_fp8_block_train_cast_weight(x.data_ptr(), p(wq), p(winv), p(wqt), p(winvt), R_, C, st))
        bufs += [qt, invt, q2, inv2, qt2, invt2, wq, winv, wqt, winvt]
    torch.cuda.synchronize()
    for b in bufs:
        assert not b.guard_problems(), b.guard_problems()
    rq, rinv = ref_rows(name)
    np.testing.assert_array_equal(by(q).reshape(R_, C), rq)
    np.testing.assert_array_equal(by(inv).view(np.uint32), _u32(rinv).reshape(-1))
    if cols:
        cq, cinv = ref_cols(name)
        np.testing.assert_array_equal(by(qt).reshape(C, R_), cq)
        np.testing.assert_array_equal(by(invt).view(np.uint32), _u32(cinv).reshape(-1))
        for one, two in ((q2, q), (inv2, inv), (qt2, qt), (invt2, invt)):
            np.testing.assert_array_equal(by(one), by(two))
        bq, binv = ref_weight(name)
        np.testing.assert_array_equal(by(wq).reshape(R_, C), bq)
        np.testing.assert_array_equal(by(wqt).reshape(C, R_), bq.T)
        np.testing.assert_array_equal(by(winv).view(np.uint32), _u32(binv).reshape(-1))
        np.testing.assert_array_equal(by(winvt).view(np.uint32), _u32(binv.T).reshape(-1))


# ---- the weight-gradient GEMM ------------------------------------------------------------------------------------------------------------
def _run_wgrad(g_t, g_inv, x_t, x_inv):
    """The C entry into a guarded, poisoned output."""
    N, M = g_t.shape
    K = x_t.shape[0]
    buf = _parity.Guarded(N, K, torch.bfloat16, torch.device(DEV, 0))
    g, gi, x, xi = _t(g_t), _t(g_inv), _t(x_t), _t(x_inv)
    _lib.check(_lib.lib().ao_fp8_block_mm_wgrad(g.data_ptr(), gi.data_ptr(), x.data_ptr(), xi.data_ptr(), buf.out.data_ptr(), M, N, K,
                                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return buf


def _exact_operands(M, N, K, seed):
    """Integer e4m3 codes |q| <= 15, power-of-two reciprocals that differ per (mb, n) and per (mb, k) within 2^7 of one another: every
    partial sum, in any order, is exact in fp32 (asserted below), so the output bits are the chain's whatever the kernel's order."""
    from oracle import fp8_ref

    g = np.random.default_rng(seed)
    mb = M // 128
    g_t = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (N, M)).astype(np.float32))
    x_t = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (K, M)).astype(np.float32))
    g_inv = np.exp2(g.integers(-2, 2, (mb, N))).astype(np.float32)
    x_inv = np.exp2(g.integers(-2, 3, (mb, K))).astype(np.float32)
    _, S = R.wgrad_f64(g_t, g_inv, x_t, x_inv)
    assert S.max() / 2.0 ** -4 < 2.0 ** 24, "the sums of this case are not exact in fp32 in every order"
    assert g_inv.max() * x_inv.max() / (g_inv.min() * x_inv.min()) <= 2.0 ** 7
    assert len(np.unique(g_inv)) > 1 and len(np.unique(x_inv)) > 1
    return g_t, g_inv, x_t, x_inv


@pytest.mark.parametrize("M,N,K", WGRAD_SHAPES)
def test_wgrad_exact_sums_pin_every_scale_index(M, N, K):
    ops_ = _exact_operands(M, N, K, 2000 + M + N + K)
    ref = R.wgrad_chain_bits(*ops_)
    _parity.check(_run_wgrad(*ops_), ref_bits=_t(ref.view(np.int16)))
    assert len(np.unique(ref)) > min(N * K, 64) // 2  # the outputs tell the elements apart
    # the op gives the entry's bits
    out = ops.fp8_block_mm_wgrad(_t(ops_[0]).view(torch.float8_e4m3fn), _t(ops_[1]), _t(ops_[2]).view(torch.float8_e4m3fn), _t(ops_[3]))
    np.testing.assert_array_equal(_bits(out), ref)


@pytest.mark.parametrize("scaled", ["g", "x"])
def test_wgrad_one_hot_operands_pin_the_lane_map(scaled):
    """One non-zero code per operand and one non-unit scale: the product lands on (n, k) alone, whatever the position in the tile, the
    wave, the fragment and the token block."""
    from oracle import fp8_ref

    M, N, K = 256, 256, 256
    two, three = (int(fp8_ref.f32_to_e4m3(np.array([v], dtype=np.float32))[0]) for v in (2.0, 3.0))
    for n, k, m in ((0, 0, 0), (5, 77, 130), (64, 17, 15), (127, 128, 255), (200, 3, 64), (255, 255, 79), (131, 196, 16), (67, 68, 144)):
        g_t, x_t = np.zeros((N, M), dtype=np.uint8), np.zeros((K, M), dtype=np.uint8)
        g_inv, x_inv = np.ones((M // 128, N), dtype=np.float32), np.ones((M // 128, K), dtype=np.float32)
        g_t[n, m], x_t[k, m] = two, three
        (g_inv if scaled == "g" else x_inv)[m // 128, n if scaled == "g" else k] = 0.5
        buf = _run_wgrad(g_t, g_inv, x_t, x_inv)
        want = np.zeros((N, K), dtype=np.float32)
        want[n, k] = 3.0
        _parity.check(buf, ref_bits=_t(R.bf16.to_bits(want).view(np.int16)))


@functools.lru_cache(maxsize=None)
def gaussian_case(M, N, K):
    """Column casts of Gaussian grad_output [M, N] and x [M, K] through the real casts, with the float64 reference (made once)."""
    g = torch.Generator().manual_seed(3000 + M + N + K)
    go = (torch.randn(M, N, generator=g) * 0.01 * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).to(torch.bfloat16)
    x = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).to(torch.bfloat16)
    _, (g_t, g_inv) = ops.fp8_block_train_cast(go.to(DEV), rows=False, cols=True)
    _, (x_t, x_inv) = ops.fp8_block_train_cast(x.to(DEV), rows=False, cols=True)
    case = tuple(a.cpu().numpy() for a in (g_t.view(torch.uint8), g_inv, x_t.view(torch.uint8), x_inv))
    np.testing.assert_array_equal(case[0], R.cast_cols(_bits(go))[0])
    return case, R.wgrad_f64(*case)


@pytest.mark.parametrize("M,N,K", WGRAD_SHAPES)
def test_wgrad_gaussian_operands_meet_the_float64_sum(M, N, K):
    case, (y, S) = gaussian_case(M, N, K)
    buf = _run_wgrad(*case)
    ref64, S = _t(y), _t(S)
    eq = (buf.out == _parity.oracle_round(ref64, torch.bfloat16)).double().mean().item()
    print("wgrad (%d, %d, %d): k_needed %.1f, equal fraction %.4f" % (M, N, K, _parity.k_needed(buf.out, ref64, S, torch.bfloat16), eq))
    _parity.check(buf, ref64=ref64, S=S, K=M, k_floor=K_FLOOR, equal=EQUAL)


def test_cast_and_wgrad_can_be_captured_in_a_graph():
    """The cast (both directions) and the weight gradient on one stream under torch.cuda.graph, replayed once: the eager run's bits."""
    G = fixture()
    go, x = _bf16(cast_input("go")).to(DEV), _bf16(cast_input("x")).to(DEV)

    def step():
        rows, (g_t, g_inv) = ops.fp8_block_train_cast(go, rows=True, cols=True)
        _, (x_t, x_inv) = ops.fp8_block_train_cast(x, rows=False, cols=True)
        return rows, ops.fp8_block_mm_wgrad(g_t, g_inv, x_t, x_inv)

    eager_rows, eager = step()  # (also warms the allocator's pools and the kernel's LDS opt-in)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rows, out = step()
        g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(out), _bits(eager))
    np.testing.assert_array_equal(_u8(rows[0]), G["go_row_q"])
    np.testing.assert_array_equal(_u32(rows[1]), _u32(eager_rows[1]))
    assert tuple(out.shape) == (128, 256) and bool(out.any())


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
def run(freeze=None):
    """(out, grad_input, grad_weight) of one forward + backward on the fixture's tensors: a 3-D input, a non-contiguous grad_output."""
    x, w, go = _operands(freeze)
    y = fp8_blockwise_mm.apply(x, w, 128)
    y.backward(_strided(go))
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (2, 128, 128)
    return y.detach(), x.grad, w.grad


def test_the_function_is_the_gemms_on_hand_made_casts():
    G = fixture()
    N, K = G["w"].shape
    x, w, go = (_bf16(G[k]).to(DEV) for k in ("x", "w", "go"))
    x, go = x.reshape(-1, K), go.reshape(-1, N)
    y, gi, gw = run()
    (xq, xi), (xt, xti) = ops.fp8_block_train_cast(x, rows=True, cols=True)
    (wq, wi), (wt, wti) = ops.fp8_block_train_cast_weight(w, transposed=None)
    (gq, gqi), (gt, gti) = ops.fp8_block_train_cast(go, rows=True, cols=True)
    np.testing.assert_array_equal(_bits(y).reshape(-1, N), _bits(ops.fp8_block_mm(xq, xi, wq, wi)))
    assert tuple(gi.shape) == (2, 128, K) and gi.dtype == torch.bfloat16
    np.testing.assert_array_equal(_bits(gi).reshape(-1, K), _bits(ops.fp8_block_mm(gq, gqi, wt, wti)))
    assert tuple(gw.shape) == (N, K) and gw.dtype == torch.bfloat16
    np.testing.assert_array_equal(_bits(gw), _bits(ops.fp8_block_mm_wgrad(gt, gti, xt, xti)))
    assert bool(y.any()) and bool(gi.any()) and bool(gw.any())


def _counted(names):
    """Wrap the named ops: (calls, restore); calls collects (name, args' shapes, kwargs)."""
    calls, real = [], {n: getattr(ops, n) for n in names}

    def wrap(n):
        def f(*a, **kw):
            calls.append((n, tuple(tuple(t.shape) for t in a if isinstance(t, torch.Tensor)), kw))
            return real[n](*a, **kw)
        return f

    for n in names:
        setattr(ops, n, wrap(n))
    return calls, lambda: [setattr(ops, n, real[n]) for n in names]


def test_a_frozen_operand_skips_its_gemm_and_its_casts():
    full = run()
    y, gi, gw = run(freeze="weight")
    assert gw is None
    np.testing.assert_array_equal(_bits(gi), _bits(full[1]))
    np.testing.assert_array_equal(_bits(y), _bits(full[0]))
    y, gi, gw = run(freeze="input")
    assert gi is None
    np.testing.assert_array_equal(_bits(gw), _bits(full[2]))
    calls, restore = _counted(("fp8_block_train_cast", "fp8_block_train_cast_weight", "fp8_block_mm", "fp8_block_mm_wgrad"))
    try:
        for freeze in ("weight", "input", None):
            x, w, go = _operands(freeze)
            y = fp8_blockwise_mm.apply(x, w, 128)
            del calls[:]
            y.backward(go)
            names = [c[0] for c in calls]
            casts = [c[2] for c in calls if c[0] == "fp8_block_train_cast"]
            if freeze == "weight":  # grad_input only: no column cast of anything, no wgrad launch
                assert names.count("fp8_block_mm_wgrad") == 0 and names.count("fp8_block_mm") == 1, calls
                assert casts == [dict(rows=True, cols=False)] and names.count("fp8_block_train_cast_weight") == 1, calls
            elif freeze == "input":  # grad_weight only: no row cast, no weight cast, no fp8_block_mm
                assert names.count("fp8_block_mm") == 0 and names.count("fp8_block_train_cast_weight") == 0, calls
                assert names.count("fp8_block_mm_wgrad") == 1 and casts == [dict(rows=False, cols=True)] * 2, calls
            else:  # both: grad_output is cast in both directions by ONE call
                assert casts == [dict(rows=True, cols=True), dict(rows=False, cols=True)], calls
                assert names.count("fp8_block_mm") == 1 and names.count("fp8_block_mm_wgrad") == 1, calls
    finally:
        restore()


def test_130_tokens_run_forward_and_grad_input_with_the_weight_frozen():
    G = fixture()
    x = _bf16(G["x"]).reshape(-1, 256)[:130].contiguous().to(DEV).requires_grad_(True)
    w = _bf16(G["w"]).to(DEV)
    go = _bf16(G["go"]).reshape(-1, 128)[:130].contiguous().to(DEV)
    y = fp8_blockwise_mm.apply(x, w, 128)
    y.backward(go)
    (xq, xi), _ = ops.fp8_block_train_cast(x.detach())
    wq, wi = ops.fp8_block_train_cast_weight(w)
    np.testing.assert_array_equal(_bits(y), _bits(ops.fp8_block_mm(xq, xi, wq, wi)))
    (gq, gqi), _ = ops.fp8_block_train_cast(go)
    wt, wti = ops.fp8_block_train_cast_weight(w, transposed=True)
    np.testing.assert_array_equal(_bits(x.grad), _bits(ops.fp8_block_mm(gq, gqi, wt, wti)))
    assert tuple(x.grad.shape) == (130, 256) and bool(x.grad.any())
    with pytest.raises(AssertionError, match="M=130 tokens must be a multiple of 128"):
        fp8_blockwise_mm.apply(x, w.clone().requires_grad_(True), 128)


def test_under_no_grad_nothing_is_saved():
    x, w, _ = _operands()
    packed = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(tuple(t.shape)) or t, lambda t: t):
        with torch.no_grad():
            quiet = fp8_blockwise_mm.apply(x, w, 128)
        assert packed == [] and not quiet.requires_grad and quiet.grad_fn is None
        loud = fp8_blockwise_mm.apply(x, w, 128)
        assert sorted(packed) == [(2, 128, 256), (128, 256)] and loud.requires_grad
    np.testing.assert_array_equal(_bits(quiet), _bits(run()[0]))
    np.testing.assert_array_equal(_bits(loud), _bits(run()[0]))


def _two_layers():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(256, 128, bias=False), nn.Linear(128, 64, bias=True)).to(torch.bfloat16).to(DEV)


def test_quantize_gives_the_bits_of_the_model_built_from_from_float():
    model, plain = _two_layers(), _two_layers()
    weight = model[0].weight
    quantize_(model, Float8BlockwiseLinearConfig(), filter_fn=lambda m, fqn: isinstance(m, nn.Linear) and fqn == "0")
    assert type(model[0]) is Float8BlockwiseLinear and type(model[1]) is nn.Linear and model[0].weight is weight
    ref = nn.Sequential(Float8BlockwiseLinear.from_float(plain[0]), plain[1])
    x0 = _operands()[0].detach()
    torch.manual_seed(1)
    go = torch.randn(2, 128, 64, device=DEV).to(torch.bfloat16)
    outs = []
    for m in (ref, model):
        x = x0.clone().requires_grad_(True)
        y = m(x)
        y.backward(go)
        outs.append((y, x.grad))
    assert outs[1][0].dtype == torch.bfloat16 and tuple(outs[1][0].shape) == (2, 128, 64)
    np.testing.assert_array_equal(_bits(outs[1][0]), _bits(outs[0][0]))
    np.testing.assert_array_equal(_bits(outs[1][1]), _bits(outs[0][1]))
    for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and bool(p.grad.any()), name
        np.testing.assert_array_equal(_bits(p.grad), _bits(q.grad), err_msg=name)
    # the swapped layer is the Function on the shared weight
    np.testing.assert_array_equal(_bits(model[0](x0)), _bits(fp8_blockwise_mm.apply(x0, weight, 128)))


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------------
def _sqnr(y, ref):
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return 10 * np.log10(np.sum(ref ** 2) / np.sum((y - ref) ** 2))


def _f64(t):
    return t.detach().double().cpu().numpy()


def _linear_runs(go):
    """((out, grad_input, grad_weight) of Float8BlockwiseLinear, the same of a bf16 nn.Linear) on the fixture's x and w; go None:
    y.sum().backward()."""
    G = fixture()
    res = []
    for blockwise in (True, False):
        lin = nn.Linear(256, 128, bias=False).to(torch.bfloat16).to(DEV)
        with torch.no_grad():
            lin.weight.copy_(_bf16(G["w"]).to(DEV))
        if blockwise:
            lin = Float8BlockwiseLinear.from_float(lin)
        x = _bf16(G["x"]).to(DEV).requires_grad_(True)
        y = lin(x)
        if go is None:
            y.sum().backward()
        else:
            y.backward(go)
        res.append((y.detach(), x.grad, lin.weight.grad))
    return res


def test_sqnr_against_a_bf16_linear_meets_the_references_bars():
    """test/prototype/blockwise_fp8_training/test_blockwise_linear.py: y.sum().backward() against bf16 nn.Linear; >= 25 dB on the output,
    >= 30 dB on each gradient."""
    ours, bf = _linear_runs(None)
    got = [_sqnr(_f64(a), _f64(b)) for a, b in zip(ours, bf)]
    print("SQNR vs bf16 nn.Linear, y.sum().backward(): out %.2f dB, grad_input %.2f dB, grad_weight %.2f dB" % tuple(got))
    assert got[0] >= 25.0 and got[1] >= 30.0 and got[2] >= 30.0


def test_sqnr_with_a_random_grad_output_stays_with_the_float64_emulation():
    """The fixture's random grad_output: each SQNR against the bf16 nn.Linear may lie at most 0.25 dB below that of the restatement's
    float64 emulation (the same casts, exact sums) against the same bf16 results -- an fp32 chain against a float64 sum is far below the
    quantisation noise."""
    G = fixture()
    ours, bf = _linear_runs(_bf16(G["go"]).to(DEV))
    emu = R.linear_emulation(G["x"].reshape(-1, 256), G["w"], G["go"].reshape(-1, 128))
    got = [_sqnr(_f64(a).reshape(e.shape), _f64(b).reshape(e.shape)) for a, b, e in zip(ours, bf, emu)]
    want = [_sqnr(e, _f64(b).reshape(e.shape)) for b, e in zip(bf, emu)]
    print("SQNR vs bf16 nn.Linear, random grad_output: out %.2f dB, grad_input %.2f dB, grad_weight %.2f dB "
          "(float64 emulation: %.2f / %.2f / %.2f dB)" % (*got, *want))
    for g, w_ in zip(got, want):
        assert g >= w_ - 0.25
