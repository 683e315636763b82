"""GPU: blockwise float8 training of the MoE grouped GEMM -- the 3-D weight cast against the 2-D cast per expert, byte for byte; the
grouped weight-gradient GEMM against the dense one (bit-exact identities on exact sums: one group, aligned groups, unaligned groups as
masked codes, bad offsets inside a guarded output, one-hot operands on either side of a group boundary) and against float64 on Gaussian
operands; the autograd Function against the ops composed by hand (bit-equal), frozen operands, no_grad, graph capture; and both cases of
the reference's test against the fixture recorded from the reference's torch functions and against bf16 torch._grouped_mm autograd.

K_FLOOR and EQUAL are the dense weight gradient's (tests/test_blockwise_fp8_training_gpu.py), unchanged: conditions, not targets.  The
Gaussian case and the SQNR cases print their figures before they assert (profiles/pytest_gpu_fp8_block_grouped_training.log).
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import _parity
import blockwise_fp8_training_ref as R
import fp8_block_grouped_training_ref as G
from ao_amd import _lib, ops
from ao_amd.prototype.blockwise_fp8_grouped_training import (
    _Float8BlockwiseGroupedMM,
    _to_fp8_blockwise_then_emulated_scaled_grouped_mm,
    _to_fp8_blockwise_then_scaled_grouped_mm,
)
from ao_amd.prototype.mx import pad_token_groups, unpad_token_groups

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
K_FLOOR = 896
EQUAL = 0.95
F8 = torch.float8_e4m3fn


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    return _load("make_golden_fp8_block_grouped_training").load()


@functools.lru_cache(maxsize=None)
def dense_fixture():
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


def _offs(o):
    return torch.tensor(list(o), dtype=torch.int32, device=DEV)


def _same(got, want):
    """(codes, inv) tensors, bit for bit"""
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous()
    np.testing.assert_array_equal(_u8(got[0]), _u8(want[0]))
    np.testing.assert_array_equal(_u32(got[1]), _u32(want[1]))


# ---- the 3-D weight cast -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weight_stack():
    """bf16 [3, 256, 384]: Gaussian experts whose rows span 2^-6 .. 2^6; expert 1 holds the 2-D fixture's edge tensor (zero blocks, the
    largest bf16, block maxima in a block's last row and column) in its first 256 columns."""
    g = torch.Generator().manual_seed(41)
    w = (torch.randn(3, 256, 384, generator=g) * torch.exp2(torch.randint(-6, 7, (3, 256, 1), generator=g).float())).to(torch.bfloat16)
    w[1, :, :256] = _bf16(dense_fixture()["edge"])
    return w.to(DEV)


@pytest.mark.parametrize("transposed", [False, True, None])
def test_the_3d_cast_is_the_2d_cast_of_every_expert(transposed):
    w = weight_stack()
    got = ops.fp8_block_train_cast_weight_3d(w, transposed=transposed)
    pairs = got if transposed is None else (got,)
    shapes = {False: ((3, 256, 384), (3, 2, 3)), True: ((3, 384, 256), (3, 3, 2))}
    for pair, t in zip(pairs, (False, True) if transposed is None else (transposed,)):
        assert (tuple(pair[0].shape), tuple(pair[1].shape)) == shapes[t] and pair[0].dtype == F8 and pair[1].dtype == torch.float32
        for e in range(3):
            _same((pair[0][e].contiguous(), pair[1][e].contiguous()), ops.fp8_block_train_cast_weight(w[e], transposed=t))
        assert not bool(((pair[0].view(torch.uint8) & 0x7F) == 0x7F).any())
    if not transposed:  # the plain pair is the 2-D cast of the [E N, K] view
        q, inv = pairs[0]
        _same((q.view(768, 384), inv.view(6, 3)), ops.fp8_block_train_cast_weight(w.view(768, 384)))


def test_the_3d_cast_entry_stays_inside_its_outputs_and_an_empty_stack_launches_nothing():
    w = weight_stack()
    E, N, K = w.shape
    dev = torch.device(DEV, 0)
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    F = lambda n: _parity.Guarded(1, n, torch.float32, dev)  # noqa: E731
    B = lambda n: _parity.Guarded(1, n // 2, torch.bfloat16, dev)  # noqa: E731  (n bytes)
    by = lambda b: b.bits().contiguous().view(torch.uint8).reshape(-1).cpu().numpy()  # noqa: E731
    p = lambda b: b.out.data_ptr()  # noqa: E731
    blocks = E * N * K // 16384
    q, inv, qt, invt, q1, inv1, qt1, invt1 = B(E * N * K), F(blocks), B(E * N * K), F(blocks), B(E * N * K), F(blocks), B(E * N * K), F(blocks)
    _lib.check(lib.ao_fp8_block_train_cast_weight_3d(w.data_ptr(), p(q), p(inv), p(qt), p(invt), E, N, K, st))
    _lib.check(lib.ao_fp8_block_train_cast_weight_3d(w.data_ptr(), p(q1), p(inv1), None, None, E, N, K, st))
    _lib.check(lib.ao_fp8_block_train_cast_weight_3d(w.data_ptr(), None, None, p(qt1), p(invt1), E, N, K, st))
    torch.cuda.synchronize()
    for b in (q, inv, qt, invt, q1, inv1, qt1, invt1):
        assert not b.guard_problems(), b.guard_problems()
    (wq, wi), (wt, wti) = ops.fp8_block_train_cast_weight_3d(w, transposed=None)
    for one, two, want in ((q, q1, _u8(wq)), (qt, qt1, _u8(wt)), (inv, inv1, _u32(wi).view(np.uint8)), (invt, invt1, _u32(wti).view(np.uint8))):
        np.testing.assert_array_equal(by(one), want.reshape(-1))
        np.testing.assert_array_equal(by(two), want.reshape(-1))
    q0, i0 = ops.fp8_block_train_cast_weight_3d(w[:0])
    assert tuple(q0.shape) == (0, 256, 384) and tuple(i0.shape) == (0, 2, 3)


# ---- the grouped weight gradient ---------------------------------------------------------------------------------------------------------
def _run_gwgrad(g_t, g_inv, x_t, x_inv, offs):
    """The C entry into a guarded, poisoned output: (the buffer over [E N, K], E)."""
    N, M = g_t.shape
    K = x_t.shape[0]
    E = 1 if offs is None else len(offs)
    buf = _parity.Guarded(E * N, K, torch.bfloat16, torch.device(DEV, 0))
    g, gi, x, xi = _t(g_t), _t(g_inv), _t(x_t), _t(x_inv)
    o = None if offs is None else _offs(offs)
    _lib.check(_lib.lib().ao_fp8_block_grouped_mm_wgrad(g.data_ptr(), gi.data_ptr(), x.data_ptr(), xi.data_ptr(),
                                                        None if o is None else o.data_ptr(), buf.out.data_ptr(), M, N, K, E,
                                                        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return buf


def _dense(g_t, g_inv, x_t, x_inv):
    """ops.fp8_block_mm_wgrad on numpy operands -> bf16 bits [N, K]"""
    return _bits(ops.fp8_block_mm_wgrad(_t(g_t).view(F8), _t(g_inv), _t(x_t).view(F8), _t(x_inv)))


def _op(case, offs):
    g_t, g_inv, x_t, x_inv = case
    return ops.fp8_block_grouped_mm_wgrad(_t(g_t).view(F8), _t(g_inv), _t(x_t).view(F8), _t(x_inv), None if offs is None else _offs(offs))


EXACT_SHAPES = [(512, 256, 128), (512, 128, 256)]  # (M, N, K) and its transpose-sized twin


@functools.lru_cache(maxsize=None)
def exact_case(M, N, K):
    return G.exact_operands(M, N, K, 5000 + N)


@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_one_group_of_every_token_is_the_dense_weight_gradient(M, N, K):
    case = exact_case(M, N, K)
    want = _dense(*case)
    np.testing.assert_array_equal(want, R.wgrad_chain_bits(*case))
    for offs in (None, (M,)):
        out = _op(case, offs)
        assert tuple(out.shape) == (1, N, K) and out.dtype == torch.bfloat16
        np.testing.assert_array_equal(_bits(out)[0], want)
        _parity.check(_run_gwgrad(*case, offs), ref_bits=_t(want.view(np.int16)))


@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_aligned_groups_are_the_dense_weight_gradient_of_their_slices(M, N, K):
    """An empty group, a one-block group, a two-block group and one more: each the dense GEMM on contiguous copies of the group's codes
    and on its rows of the scales."""
    g_t, g_inv, x_t, x_inv = case = exact_case(M, N, K)
    offs = (128, 128, 384, 512)
    buf = _run_gwgrad(*case, offs)
    got = _bits(buf.out).reshape(4, N, K)
    want = np.zeros_like(got)
    for e, (lo, hi) in enumerate(G.bounds(offs, M)):
        if hi > lo:
            b0, b1 = lo // 128, hi // 128
            want[e] = _dense(np.ascontiguousarray(g_t[:, lo:hi]), g_inv[b0:b1], np.ascontiguousarray(x_t[:, lo:hi]), x_inv[b0:b1])
    _parity.check(buf, ref_bits=_t(want.reshape(4 * N, K).view(np.int16)))
    assert not got[1].any() and got[0].any() and got[2].any() and got[3].any()
    np.testing.assert_array_equal(_bits(_op(case, offs)), want)


@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_unaligned_groups_are_the_dense_weight_gradient_of_masked_codes(M, N, K):
    """Group ends inside a token block, 12 tokens in no group: as numbers, the dense GEMM over all M with every foreign token's code 0;
    and the helper's fp32 chain, bit for bit."""
    g_t, g_inv, x_t, x_inv = case = exact_case(M, N, K)
    offs = (129, 384, 500)
    buf = _run_gwgrad(*case, offs)
    assert not buf.guard_problems(), buf.guard_problems()
    got = buf.out.float().cpu().numpy().reshape(3, N, K)
    for e, (lo, hi) in enumerate(G.bounds(offs, M)):
        dense = _dense(G.masked(g_t, lo, hi), g_inv, G.masked(x_t, lo, hi), x_inv)
        assert np.array_equal(got[e], R.bf16.from_bits(dense).astype(np.float32)), "group %d" % e
    chain = G.grouped_wgrad_chain_bits(*case, offs)
    _parity.check(buf, ref_bits=_t(chain.reshape(3 * N, K).view(np.int16)))
    # the 12 tokens past offs[-1] reach nothing: the three groups and they add up to the dense sum
    y_all = R.wgrad_f64(*case)[0]
    y_tail = R.wgrad_f64(G.masked(g_t, 500, 512), g_inv, G.masked(x_t, 500, 512), x_inv)[0]
    y_sum = sum(y for y, _ in G.grouped_wgrad_f64(*case, offs))
    np.testing.assert_allclose(y_sum + y_tail, y_all, rtol=0, atol=1e-9)
    assert np.abs(y_tail).max() > 0


def test_bad_offsets_stay_inside_the_output_and_empty_groups_are_zeros():
    """A first empty group, an end past M and a decreasing pair: offs is clamped to [0, M]."""
    M, N, K = EXACT_SHAPES[0]
    case = exact_case(M, N, K)
    offs = (0, 600, 300)
    buf = _run_gwgrad(*case, offs)
    want = np.zeros((3, N, K), dtype=np.uint16)
    want[1] = _dense(*case)  # [0, 600) clamped: every token
    _parity.check(buf, ref_bits=_t(want.reshape(3 * N, K).view(np.int16)))
    assert G.bounds(offs, M) == [(0, 0), (0, 512), (512, 512)]
    out = ops.fp8_block_grouped_mm_wgrad(_t(case[0][:, :0]).view(F8), _t(case[1][:0]), _t(case[2][:, :0]).view(F8), _t(case[3][:0]),
                                         _offs((0, 0)))  # M == 0: zeros
    assert tuple(out.shape) == (2, N, K) and not bool(out.any())


@pytest.mark.parametrize("scaled", ["g", "x"])
def test_one_hot_operands_land_in_the_right_expert_only(scaled):
    """One non-zero code per operand, one non-unit scale, the hot token on either side of the group boundary at token 129 (inside the
    second token block): the product lands on (e, n, k) alone."""
    M, N, K = 256, 256, 256
    offs = (129, 256)
    two, three = (int(R.fp8_ref.f32_to_e4m3(np.array([v], dtype=np.float32))[0]) for v in (2.0, 3.0))
    for n, k, m in ((0, 0, 0), (5, 77, 128), (64, 17, 129), (127, 128, 255), (200, 3, 127), (255, 255, 130), (131, 196, 143), (67, 68, 144)):
        g_t, x_t = np.zeros((N, M), dtype=np.uint8), np.zeros((K, M), dtype=np.uint8)
        g_inv, x_inv = np.ones((M // 128, N), dtype=np.float32), np.ones((M // 128, K), dtype=np.float32)
        g_t[n, m], x_t[k, m] = two, three
        (g_inv if scaled == "g" else x_inv)[m // 128, n if scaled == "g" else k] = 0.5
        buf = _run_gwgrad(g_t, g_inv, x_t, x_inv, offs)
        want = np.zeros((2, N, K), dtype=np.float32)
        want[0 if m < 129 else 1, n, k] = 3.0
        _parity.check(buf, ref_bits=_t(R.bf16.to_bits(want).reshape(2 * N, K).view(np.int16)))


@functools.lru_cache(maxsize=None)
def gaussian_case(M, N, K):
    """Column casts of Gaussian grad_output [M, N] and x [M, K] through the real casts (gaussian_case of the dense test)."""
    g = torch.Generator().manual_seed(3000 + M + N + K)
    go = (torch.randn(M, N, generator=g) * 0.01 * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).to(torch.bfloat16)
    x = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).to(torch.bfloat16)
    _, (g_t, g_inv) = ops.fp8_block_train_cast(go.to(DEV), rows=False, cols=True)
    _, (x_t, x_inv) = ops.fp8_block_train_cast(x.to(DEV), rows=False, cols=True)
    case = tuple(a.cpu().numpy() for a in (g_t.view(torch.uint8), g_inv, x_t.view(torch.uint8), x_inv))
    np.testing.assert_array_equal(case[0], R.cast_cols(_bits(go))[0])
    return case


def test_gaussian_operands_meet_the_float64_sum_per_expert():
    M, N, K = 512, 256, 128
    offs = (129, 384, 500)
    case = gaussian_case(M, N, K)
    out = _run_gwgrad(*case, offs)
    assert not out.guard_problems(), out.guard_problems()
    for e, ((lo, hi), (y, S)) in enumerate(zip(G.bounds(offs, M), G.grouped_wgrad_f64(*case, offs))):
        buf = _parity.Guarded(N, K, torch.bfloat16, torch.device(DEV, 0))
        buf.out.copy_(out.out[e * N:(e + 1) * N])
        ref64, S_ = _t(y), _t(S)
        eq = (buf.out == _parity.oracle_round(ref64, torch.bfloat16)).double().mean().item()
        print("grouped wgrad (%d, %d, %d) expert %d, tokens [%d, %d): k_needed %.1f, equal fraction %.4f"
              % (M, N, K, e, lo, hi, _parity.k_needed(buf.out, ref64, S_, torch.bfloat16), eq))
        _parity.check(buf, ref64=ref64, S=S_, K=hi - lo, k_floor=K_FLOOR, equal=EQUAL)


def test_cast_and_grouped_wgrad_can_be_captured_in_a_graph():
    """The casts (both directions) and the grouped weight gradient on one stream under torch.cuda.graph, replayed once: the eager bits."""
    ab, _, gob = G.operands("aligned")
    go, x, offs = _bf16(gob).to(DEV), _bf16(ab).to(DEV), _offs((129, 384, 500))

    def step():
        rows, (g_t, g_inv) = ops.fp8_block_train_cast(go, rows=True, cols=True)
        _, (x_t, x_inv) = ops.fp8_block_train_cast(x, rows=False, cols=True)
        return rows, ops.fp8_block_grouped_mm_wgrad(g_t, g_inv, x_t, x_inv, offs)

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
    np.testing.assert_array_equal(_u8(rows[0]), _u8(eager_rows[0]))
    assert tuple(out.shape) == (3, 256, 256) and all(bool(out[e].any()) for e in range(3))


# ---- the Function ------------------------------------------------------------------------------------------------------------------------
def _strided(t):
    """The same values, non-contiguous."""
    out = t.transpose(0, 1).contiguous().transpose(0, 1)
    assert not out.is_contiguous()
    return out


def _operands(case, freeze=None):
    """(A, B_t, grad_out, offs) of a fixture case on the device; B_t a column-major leaf as in the reference's test."""
    ab, wb, gob = G.operands(case)
    A = _bf16(ab).to(DEV).requires_grad_(freeze != "A")
    B_t = _bf16(wb).to(DEV).transpose(-2, -1).requires_grad_(freeze != "B")
    return A, B_t, _bf16(gob).to(DEV), _offs(G.CASES[case]["offs"])


@functools.lru_cache(maxsize=None)
def run(case, freeze=None, pad=None):
    """(out, grad_A, grad_B_t) of one forward + backward on a fixture case, with a non-contiguous grad_output."""
    A, B_t, go, offs = _operands(case, freeze)
    pad = G.CASES[case]["pad"] if pad is None else pad
    y = _to_fp8_blockwise_then_scaled_grouped_mm(A, B_t, offs, pad_token_groups_for_grouped_mm=pad)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (A.shape[0], 256)
    y.backward(_strided(go))
    return y.detach(), A.grad, B_t.grad


@pytest.mark.parametrize("case", list(G.CASES))
def test_the_function_is_the_ops_on_hand_made_casts(case):
    A, B_t, go, offs = (t.detach() for t in _operands(case))
    pad, M = G.CASES[case]["pad"], A.shape[0]
    y, gA, gB_t = run(case)
    W = B_t.transpose(-2, -1)
    assert W.is_contiguous()
    if pad:
        A_p, starts, ends = pad_token_groups(A, offs, 128)
        go_p = pad_token_groups(go, offs, 128)[0]
        assert A_p.shape[0] % 128 == 0 and not bool(A_p[int(ends[-1]):].any())
        unpad = lambda t: unpad_token_groups(t, offs, starts, M, 128)  # noqa: E731
    else:
        A_p, go_p, ends, unpad = A, go, offs, lambda t: t
    (aq, ai), (at, ati) = ops.fp8_block_train_cast(A_p, rows=True, cols=True)
    (wq, wi), (wt, wti) = ops.fp8_block_train_cast_weight_3d(W, transposed=None)
    (gq, gi), (gt, gti) = ops.fp8_block_train_cast(go_p, rows=True, cols=True)
    np.testing.assert_array_equal(_bits(y), _bits(unpad(ops.fp8_block_grouped_mm(aq, ai, wq, wi, ends))))
    assert tuple(gA.shape) == (M, 256) and gA.dtype == torch.bfloat16
    np.testing.assert_array_equal(_bits(gA), _bits(unpad(ops.fp8_block_grouped_mm(gq, gi, wt, wti, ends))))
    E = W.shape[0]
    assert tuple(gB_t.shape) == (E, 256, 256) and gB_t.dtype == torch.bfloat16 and gB_t.stride() == B_t.stride()
    np.testing.assert_array_equal(_bits(gB_t.transpose(-2, -1)), _bits(ops.fp8_block_grouped_mm_wgrad(gt, gti, at, ati, ends)))
    assert bool(y.any()) and bool(gA.any()) and all(bool(gB_t[e].any()) for e in range(E))
    # the emulated entry and the Function itself are the same computation
    with torch.no_grad():
        np.testing.assert_array_equal(_bits(_to_fp8_blockwise_then_emulated_scaled_grouped_mm(
            A, B_t, offs, pad_token_groups_for_grouped_mm=pad)), _bits(y))
        np.testing.assert_array_equal(_bits(_Float8BlockwiseGroupedMM.apply(A, B_t, offs, torch.bfloat16, F8, 128, pad)), _bits(y))


def test_on_aligned_groups_padding_changes_no_bit():
    plain, padded = run("aligned", pad=False), run("aligned", pad=True)
    for a, b in zip(plain, padded):
        np.testing.assert_array_equal(_bits(a), _bits(b))


def _counted(names):
    """Wrap the named ops: (calls, restore); calls collects (name, args' shapes, kwargs, result)."""
    calls, real = [], {n: getattr(ops, n) for n in names}

    def wrap(n):
        def f(*a, **kw):
            res = real[n](*a, **kw)
            calls.append((n, tuple(tuple(t.shape) for t in a if isinstance(t, torch.Tensor)), kw, res))
            return res
        return f

    for n in names:
        setattr(ops, n, wrap(n))
    return calls, lambda: [setattr(ops, n, real[n]) for n in names]


OP_NAMES = ("fp8_block_train_cast", "fp8_block_train_cast_weight_3d", "fp8_block_grouped_mm", "fp8_block_grouped_mm_wgrad")


def test_a_frozen_operand_skips_its_gemm_and_its_casts():
    full = run("padded")
    y, gA, gB = run("padded", freeze="B")
    assert gB is None
    np.testing.assert_array_equal(_bits(gA), _bits(full[1]))
    np.testing.assert_array_equal(_bits(y), _bits(full[0]))
    y, gA, gB = run("padded", freeze="A")
    assert gA is None
    np.testing.assert_array_equal(_bits(gB), _bits(full[2]))
    calls, restore = _counted(OP_NAMES)
    try:
        for freeze in ("B", "A", None):
            A, B_t, go, offs = _operands("padded", freeze)
            y = _to_fp8_blockwise_then_scaled_grouped_mm(A, B_t, offs)
            assert [c[0] for c in calls] == ["fp8_block_train_cast", "fp8_block_train_cast_weight_3d", "fp8_block_grouped_mm"], calls
            del calls[:]
            y.backward(go)
            names = [c[0] for c in calls]
            casts = [c[2] for c in calls if c[0] == "fp8_block_train_cast"]
            wcasts = [c[2] for c in calls if c[0] == "fp8_block_train_cast_weight_3d"]
            if freeze == "B":  # grad_A only: no column cast of anything, no wgrad launch
                assert names.count("fp8_block_grouped_mm_wgrad") == 0 and names.count("fp8_block_grouped_mm") == 1, calls
                assert casts == [dict(rows=True, cols=False)] and wcasts == [dict(transposed=True)], calls
            elif freeze == "A":  # grad_B only: no row cast, no weight cast, no fp8_block_grouped_mm
                assert names.count("fp8_block_grouped_mm") == 0 and wcasts == [], calls
                assert names.count("fp8_block_grouped_mm_wgrad") == 1 and casts == [dict(rows=False, cols=True)] * 2, calls
            else:  # both: grad_output is cast in both directions by ONE call
                assert casts == [dict(rows=True, cols=True), dict(rows=False, cols=True)] and wcasts == [dict(transposed=True)], calls
                assert names.count("fp8_block_grouped_mm") == 1 and names.count("fp8_block_grouped_mm_wgrad") == 1, calls
            del calls[:]
    finally:
        restore()


def test_any_token_count_runs_forward_and_grad_a_without_padding_while_b_is_frozen():
    A, B_t, go, _ = _operands("padded", freeze="B")  # M = 500
    offs = _offs((129, 384, 500))
    y = _to_fp8_blockwise_then_scaled_grouped_mm(A, B_t, offs, pad_token_groups_for_grouped_mm=False)
    y.backward(go)
    (aq, ai), _ = ops.fp8_block_train_cast(A.detach())
    (wq, wi), (wt, wti) = ops.fp8_block_train_cast_weight_3d(B_t.detach().transpose(-2, -1), transposed=None)
    np.testing.assert_array_equal(_bits(y), _bits(ops.fp8_block_grouped_mm(aq, ai, wq, wi, offs)))
    (gq, gi), _ = ops.fp8_block_train_cast(go)
    np.testing.assert_array_equal(_bits(A.grad), _bits(ops.fp8_block_grouped_mm(gq, gi, wt, wti, offs)))
    # the unpadded forward is the padded one: padding moves rows, and a row's 1 x 128 blocks do not see its neighbours
    np.testing.assert_array_equal(_bits(y), _bits(run("padded")[0]))
    np.testing.assert_array_equal(_bits(A.grad), _bits(run("padded")[1]))
    with pytest.raises(AssertionError, match="M=500 tokens must be a multiple of 128"):
        _to_fp8_blockwise_then_scaled_grouped_mm(A, B_t.detach().requires_grad_(True), offs, pad_token_groups_for_grouped_mm=False)


def test_under_no_grad_nothing_is_saved():
    A, B_t, _, offs = _operands("padded")
    packed = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(tuple(t.shape)) or t, lambda t: t):
        with torch.no_grad():
            quiet = _to_fp8_blockwise_then_scaled_grouped_mm(A, B_t, offs)
        assert packed == [] and not quiet.requires_grad and quiet.grad_fn is None
        loud = _to_fp8_blockwise_then_scaled_grouped_mm(A, B_t, offs)
        assert sorted(packed) == [(3,), (3,), (3,), (3, 256, 256), (896, 256)] and loud.requires_grad
    np.testing.assert_array_equal(_bits(quiet), _bits(run("padded")[0]))
    np.testing.assert_array_equal(_bits(loud), _bits(run("padded")[0]))


# ---- against the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(G.CASES))
def test_every_cast_the_function_makes_is_the_recorded_one(case):
    F = fixture()
    A, B_t, go, offs = _operands(case)
    calls, restore = _counted(OP_NAMES[:2])
    try:
        _to_fp8_blockwise_then_scaled_grouped_mm(A, B_t, offs, pad_token_groups_for_grouped_mm=G.CASES[case]["pad"]).backward(go)
    finally:
        restore()
    res = [c[3] for c in calls]
    assert [c[0] for c in calls] == ["fp8_block_train_cast", "fp8_block_train_cast_weight_3d"] * 2 + ["fp8_block_train_cast"], calls
    made = {"a_row": res[0][0], "w": res[1], "go_row": res[2][0], "go_col": res[2][1], "w_t": res[3], "a_col": res[4][1]}
    for name, (q, inv) in made.items():
        np.testing.assert_array_equal(G.sha(_u8(q)), F["%s_%s_q_sha" % (case, name)], err_msg=name)
        np.testing.assert_array_equal(_u32(inv), _u32(F["%s_%s_inv" % (case, name)]), err_msg=name)


@pytest.mark.parametrize("case", list(G.CASES))
def test_each_result_is_at_least_as_close_to_the_exact_product_as_the_references_emulation(case):
    """The reference's emulation rounds both dequantized operands to bf16, so its result is the yardstick, not the truth: for out, grad_A
    and grad_B the SQNR of ours against the float64 product of the recorded dequantized casts must be at least the reference's recorded
    SQNR against the same product -- over the whole tensor, and over the rows of the reference's result that the fixture keeps."""
    F, spec = fixture(), G.CASES[case]
    ab, wb, gob = G.operands(case)
    casts, starts, ends = G.function_casts(ab, wb, gob, spec["offs"], spec["pad"])
    ref64 = G.function_f64(casts, spec["offs"], starts, ends, ab.shape[0])
    y, gA, gB_t = run(case)
    ours = (y, gA, gB_t.transpose(-2, -1))
    for name, t, r in zip(("out", "grad_a", "grad_w"), ours, ref64):
        np.testing.assert_allclose(np.sum(r ** 2), float(F["%s_%s_energy" % (case, name)]), rtol=1e-12)
        t = t.double().cpu().numpy()
        got, want = G.sqnr(t, r), float(F["%s_%s_ref_sqnr" % (case, name)])
        theirs = R.bf16.from_bits(F["%s_%s_sample" % (case, name)]).astype(np.float64)
        got_s, want_s = G.sqnr(G.sample(t), G.sample(r)), G.sqnr(theirs, G.sample(r))
        print("%s %s against the float64 product of the recorded casts: ours %.2f dB, the reference's emulation %.2f dB; on the recorded "
              "rows %.2f dB and %.2f dB" % (case, name, got, want, got_s, want_s))
        assert got >= want and got_s >= want_s


@pytest.mark.parametrize("case", list(G.CASES))
def test_sqnr_against_bf16_grouped_mm_autograd_meets_the_references_bars(case):
    """test/prototype/moe_training/test_fp8_blockwise_grouped_mm.py:44-74: randn operands, out.float().square().mean().backward() on
    both sides; out >= 27 dB, grad_A >= 26 dB, grad_B >= 26 dB."""
    spec = G.CASES[case]
    offs = _offs(spec["offs"])
    E, M, K, N = len(spec["offs"]), spec["offs"][-1], 256, 256
    g = torch.Generator().manual_seed(0)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV).requires_grad_(True)
    B_t = torch.randn(E, N, K, generator=g).to(torch.bfloat16).to(DEV).transpose(-2, -1).requires_grad_(True)
    A_ref, B_t_ref = A.detach().clone().requires_grad_(True), B_t.detach().clone().requires_grad_(True)
    out = _to_fp8_blockwise_then_emulated_scaled_grouped_mm(A, B_t, offs, pad_token_groups_for_grouped_mm=spec["pad"])
    ref = torch._grouped_mm(A_ref, B_t_ref, offs=offs, out_dtype=torch.bfloat16)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    out.float().square().mean().backward()
    ref.float().square().mean().backward()
    f64 = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    got = [G.sqnr(f64(a), f64(b)) for a, b in ((out, ref), (A.grad, A_ref.grad), (B_t.grad, B_t_ref.grad))]
    print("%s SQNR vs bf16 torch._grouped_mm autograd: out %.2f dB, grad_A %.2f dB, grad_B %.2f dB" % (case, *got))
    assert got[0] >= 27.0 and got[1] >= 26.0 and got[2] >= 26.0
