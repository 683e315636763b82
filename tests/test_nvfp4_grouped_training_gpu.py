"""NVFP4 MoE grouped-GEMM training on the GPU: the grouped casts against the restatement (tests/nvfp4_train_ref.py) per
group slice, the 3-D weight entries against the dense ops, both GEMMs against float64 sums of the decoded codes, and _NVFP4GroupedMM
against the restated chain.  Every case prints its figures before it asserts (profiles/pytest_gpu_nvfp4_grouped_training.log)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nvfp4_ref as R  # noqa: E402
import nvfp4_train_ref as T  # noqa: E402
import test_nvfp4_training_gpu as D  # noqa: E402  (its guarded buffers, exact operands, Gaussian matrix and interval check)

pytestmark = pytest.mark.gpu

SIGN = T.DEFAULT_SIGN_VECTOR
# a 16-row group, an empty group, a group crossing a 128-row tile and a 64-token step, ends that are 16- but not 32-aligned, 16 capacity rows
OFFS = {"five": (224, [16, 48, 48, 176, 208]), "one": (224, [224]), "two": (272, [128, 272])}
WIDTHS = [(144, 80), (128, 256)]  # (N, K), ragged against the 128-tile and whole tiles


def _dev():
    return torch.device("cuda", 0)


def _offs(ends):
    return torch.tensor(ends, dtype=torch.int32, device=_dev())


def _slices(ends):
    return list(zip([0] + ends[:-1], ends))


def _ref_amax(xc, ends):
    return torch.stack([T.amaxes(xc[s:t], SIGN) if t > s else torch.zeros(2) for s, t in _slices(ends)])


def _ref_cast(xc, amax, ends, sr=()):
    """The restatement per group slice: a cast is local to a 16-row run, so group e's slice of the cast of the whole matrix under amax[e]
    is the cast of its slice, under SR with the whole output's counters.  Capacity rows are zero."""
    m, n = xc.shape
    out = [torch.zeros(r, c, dtype=torch.uint8) for r, c in ((n, m // 2), (n, m // 16), (m, n // 2), (m, n // 16))]
    for e, (s, t) in enumerate(_slices(ends)):
        if t > s:
            cq, cs, rq, rs = T.quantize_row_col(xc, amax[e], SIGN, *sr)
            out[0][:, s // 2:t // 2], out[1][:, s // 16:t // 16], out[2][s:t], out[3][s:t] = cq[:, s // 2:t // 2], cs[:, s // 16:t // 16], rq[s:t], rs[s:t]
    return out


def _grouped_cast(x, amax, ends, sr=None):
    """the grouped cast into guarded buffers -> CPU tensors (col_q, col_s, row_q, row_s)"""
    from ao_amd import ops

    m, n = x.shape
    col, row = D._pairs(n, m), D._pairs(m, n)
    seed, co, ro = (None, None, None) if sr is None else (D._i64(sr[0]), D._i64(sr[1]), D._i64(sr[2]))
    ops.nvfp4_train_quantize_row_col_grouped(x, amax, _offs(ends), SIGN, seed, co, ro, col_out=(col[0].out, col[1].out),
                                             row_out=(row[0].out, row[1].out))
    torch.cuda.synchronize()
    assert all(g.clean() for g in col + row), "a write outside the output"
    return tuple(g.out.cpu() for g in col + row)


# ---- 1, 2. the per-group amax and the grouped cast ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [144, 80, 256])
@pytest.mark.parametrize("case", list(OFFS))
def test_group_amax_and_cast_equal_the_restatement_per_slice(case, width):
    from ao_amd import ops

    m, ends = OFFS[case]
    xc = D._matrix(m, width, 7 + m + width)
    xc[ends[-1]:] = 1000.0  # capacity rows hold the tensor's largest value and reach no amax
    x = xc.to(_dev())
    want_amax = _ref_amax(xc, ends)
    amax = ops.nvfp4_train_group_amax(x, _offs(ends), SIGN)
    print(f"{case} width {width}: group amaxes {amax.cpu().tolist()}")
    assert torch.equal(amax.cpu().view(torch.int32), want_amax.view(torch.int32)), (amax.cpu(), want_amax)
    no_rht = ops.nvfp4_train_group_amax(x, _offs(ends), SIGN, want_rht=False).cpu()
    assert bool((no_rht[:, 0] == 0).all()) and torch.equal(no_rht[:, 1], want_amax[:, 1])
    got = _grouped_cast(x, amax, ends)
    D._same(got, _ref_cast(xc, want_amax, ends), f"{case} width {width} RTNE")
    assert all(int(g[ends[-1]:].sum()) == 0 for g in got[2:]) and int(got[0][:, ends[-1] // 2:].sum()) == 0 and int(got[1][:, ends[-1] // 16:].sum()) == 0


@pytest.mark.parametrize("case", ["one", "five"])
def test_grouped_cast_under_stochastic_rounding_equals_the_dense_cast(case):
    """one group, and five groups under ONE shared amax pair: the dense cast's counters and bytes (up to the zeroed capacity rows)"""
    from ao_amd import ops

    m, ends = OFFS[case]
    x = D._matrix(m, 144, 31).to(_dev())
    amax2 = ops.nvfp4_train_amax(x, SIGN)
    amax = amax2.reshape(1, 2).repeat(len(ends), 1).contiguous()
    live = ends[-1]
    for seed, off in D.SR_PAIRS:
        sr = (seed, off, off ^ 0x5A5A)
        want = [t.cpu() for t in ops.nvfp4_train_quantize_row_col(x, amax2, SIGN, D._i64(sr[0]), D._i64(sr[1]), D._i64(sr[2]))]
        got = _grouped_cast(x, amax, ends, sr)
        want = [want[0][:, :live // 2], want[1].view(torch.uint8)[:, :live // 16], want[2][:live], want[3].view(torch.uint8)[:live]]
        D._same([got[0][:, :live // 2], got[1][:, :live // 16], got[2][:live], got[3][:live]], want, f"{case} SR seed {seed:#x}")


# ---- 3. the 3-D weight amax and cast --------------------------------------------------------------------------------------------------------
def test_weight_3d_equals_the_dense_ops_per_expert():
    from ao_amd import ops

    w = torch.stack([D._matrix(144, 80, 50 + e) * 2.0 ** e for e in range(3)]).to(_dev())
    amax = ops.nvfp4_train_weight_amax_3d(w)
    got = ops.nvfp4_train_quantize_weight_3d(w, amax)
    for e in range(3):
        dense = ops.nvfp4_train_amax(w[e].contiguous(), 0, want_rht=False)[1]
        assert torch.equal(amax[e].view(torch.int32), dense.view(torch.int32))
        for g, d in zip(got, ops.nvfp4_train_quantize_weight_2d(w[e].contiguous(), dense)):
            assert torch.equal(g[e].view(torch.uint8), d.view(torch.uint8)), f"expert {e}"


# ---- 4. the GEMMs -----------------------------------------------------------------------------------------------------------------------------
def _scales(e, g, pow2):
    return torch.exp2(torch.randint(-8, 4, (e,), generator=g).float()) if pow2 else torch.rand(e, generator=g) * 0.01 + 1e-3


def _wgrad_ref(gq, gs, xq, xs, pg, px, ends):
    """per group (ref64, S) of the float64 sums of the decoded codes (an empty group: an empty sum, zeros)"""
    return [T.scaled_mm_sums(gq[:, s // 2:t // 2], gs[:, s // 16:t // 16], xq[:, s // 2:t // 2], xs[:, s // 16:t // 16], pg[e], px[e])
            for e, (s, t) in enumerate(_slices(ends))]


def _wgrad(gq, gs, xq, xs, pg, px, ends):
    from ao_amd import ops

    return ops.nvfp4_grouped_mm_wgrad(*(t.to(_dev()) for t in (gq, gs, xq, xs, pg, px)), None if ends is None else _offs(ends)).cpu()


def _operand(rows, cols, g, exact, std=1.0):
    if exact:
        return D._exact_operand(rows, cols, g)
    x = (torch.randn(rows, cols, generator=g) * std).to(torch.bfloat16)
    return T.cast(x, x.float().abs().max())


@pytest.mark.parametrize("n,k", WIDTHS)
@pytest.mark.parametrize("case", list(OFFS))
def test_wgrad_exact_sums_gaussian_casts_and_no_offs(case, n, k):
    """Exact-sum operands: bit-identical to the float64 sums.  Gaussian casts: inside the dense training GEMM's interval (_parity.bound)
    with K the group's token count.  Without offs the launch is a dense weight gradient: nvfp4_scaled_mm on the same operands, bit for bit."""
    from ao_amd import ops

    m, ends = OFFS[case]
    assert m * 144 * 16 <= 2 ** 24  # terms are multiples of 1/16, |term| <= (6 x 2)^2: every partial sum is exact in fp32
    g = torch.Generator().manual_seed(m + n)
    for exact in (True, False):
        (gq, gs), (xq, xs) = _operand(n, m, g, exact), _operand(k, m, g, exact, 0.1)
        pg, px = _scales(len(ends), g, exact), _scales(len(ends), g, exact)
        out = _wgrad(gq, gs, xq, xs, pg, px, ends)
        for e, ((ref64, S), (s, t)) in enumerate(zip(_wgrad_ref(gq, gs, xq, xs, pg, px, ends), _slices(ends))):
            if exact:
                assert torch.equal(R.bits(out[e]), R.bits(ref64.float().to(torch.bfloat16))), f"group {e} of {case}"
            else:
                D._inside(f"wgrad {case} group {e} ({t - s} tokens)", out[e], ref64, S, t - s)
        dense = ops.nvfp4_scaled_mm(*(t.to(_dev()) for t in (gq, gs, xq, xs, pg[:1], px[:1]))).cpu()
        same = R.bits(_wgrad(gq, gs, xq, xs, pg[:1], px[:1], None)[0]) == R.bits(dense)
        print(f"  no offs against nvfp4_scaled_mm ({'exact-sum' if exact else 'Gaussian'}, {m} tokens): {float(same.float().mean()):.6f} equal")
        assert bool(same.all())


@pytest.mark.parametrize("group", [1, 3])
def test_wgrad_keeps_a_neighbours_nan_scales_out(group):
    m, ends = OFFS["five"]
    g = torch.Generator().manual_seed(group)
    (gq, gs), (xq, xs) = D._exact_operand(144, m, g), D._exact_operand(80, m, g)
    pg, px = _scales(5, g, True), _scales(5, g, True)
    want = _wgrad_ref(gq, gs, xq, xs, pg, px, ends)[group][0]
    s, t = _slices(ends)[group]
    for sc in (gs, xs):  # every token outside the group under test, the capacity rows included, carries the e4m3 NaN
        sc[:, :s // 16] = 0x7F
        sc[:, t // 16:] = 0x7F
    out = _wgrad(gq, gs, xq, xs, pg, px, ends)[group]
    assert bool(torch.isfinite(out.float()).all()) and torch.equal(R.bits(out), R.bits(want.float().to(torch.bfloat16)))


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("n,k", WIDTHS)
@pytest.mark.parametrize("case", list(OFFS))
def test_scaled_grouped_mm_exact_and_gaussian(case, n, k, form):
    from ao_amd import ops

    (m, ends), e = OFFS[case], len(OFFS[case][1])
    g = torch.Generator().manual_seed(form + m)
    for exact in (True, False):
        (aq, a_s), b = _operand(m, k, g, exact), [_operand(n, k, g, exact, 0.1) for _ in range(e)]
        pa, pb = _scales(e, g, exact), _scales(e, g, exact)
        bq, bs = torch.stack([q for q, _ in b]), torch.stack([s for _, s in b])
        ops.nvfp4_grouped_mm_set_form(form)
        try:
            out = ops.nvfp4_scaled_grouped_mm(*(t.to(_dev()) for t in (aq, a_s, bq, bs)), _offs(ends), pa.to(_dev()), pb.to(_dev())).cpu()
        finally:
            ops.nvfp4_grouped_mm_set_form(0)
        assert int(out[ends[-1]:].view(torch.int16).abs().sum()) == 0
        for i, (s, t) in enumerate(_slices(ends)):
            if t == s:
                continue
            ref64, S = T.scaled_mm_sums(aq[s:t], a_s[s:t], bq[i], bs[i], pa[i], pb[i])
            if exact:
                assert torch.equal(R.bits(out[s:t]), R.bits(ref64.float().to(torch.bfloat16))), f"group {i} of {case}, form {form}"
            else:
                D._inside(f"scaled_grouped_mm form {form} group {i}", out[s:t], ref64, S, k)


# ---- 5. the Function ----------------------------------------------------------------------------------------------------------------------------
E, M, N, K = 4, 256, 144, 128
ENDS = [48, 64, 192, 256]
SEED = 0x0123456789ABCDEF


def _inputs():
    g = torch.Generator().manual_seed(17)
    return (torch.randn(M, K, generator=g).to(torch.bfloat16), (torch.randn(E, N, K, generator=g) * 0.05).to(torch.bfloat16),
            torch.randn(M, N, generator=g).to(torch.bfloat16))


def _run(xc, wc, dyc, ends, pad=False):
    from ao_amd.prototype import _to_nvfp4_rht_rs_then_scaled_grouped_mm

    x, w = xc.to(_dev()).requires_grad_(True), wc.to(_dev()).requires_grad_(True)
    torch.manual_seed(11)
    y = _to_nvfp4_rht_rs_then_scaled_grouped_mm(x, w, SIGN, D._i64(SEED), _offs(ends), pad_token_groups_for_grouped_mm=pad)
    y.backward(dyc.to(_dev()))
    torch.cuda.synchronize()
    return y.detach().cpu(), x.grad.cpu(), w.grad.cpu()


def restated_chain(xc, wc, dyc, ends, col_offset, row_offset):
    """_NVFP4GroupedMM restated: per group (ref64, S) of out, grad_A and grad_B"""
    xa, da = _ref_amax(xc, ends), _ref_amax(dyc, ends)
    wa = wc.float().abs().amax(dim=(1, 2))
    xcq, xcs, xrq, xrs = _ref_cast(xc, xa, ends)
    dcq, dcs, drq, drs = _ref_cast(dyc, da, ends, (SEED, col_offset, row_offset))
    sums = {"out": [], "grad_A": [], "grad_B": []}
    for e, (s, t) in enumerate(_slices(ends)):
        wq, ws, wtq, wts = T.quantize_weight_2d(wc[e], wa[e])
        sums["out"].append(T.scaled_mm_sums(xrq[s:t], xrs[s:t], wq, ws, T.amax_to_scale(xa[e, 1]), T.amax_to_scale(wa[e])))
        sums["grad_A"].append(T.scaled_mm_sums(drq[s:t], drs[s:t], wtq, wts, T.amax_to_scale(da[e, 1]), T.amax_to_scale(wa[e])))
        sums["grad_B"].append(T.scaled_mm_sums(dcq[:, s // 2:t // 2], dcs[:, s // 16:t // 16], xcq[:, s // 2:t // 2], xcs[:, s // 16:t // 16],
                                               T.amax_to_scale(da[e, 0]), T.amax_to_scale(xa[e, 0])))
    return sums


def fp32_grouped(xc, wc, dyc, ends):
    """fp32 torch._grouped_mm autograd on the bf16 operands"""
    x, w = xc.float().requires_grad_(True), wc.float().requires_grad_(True)
    y = torch._grouped_mm(x, w.transpose(-2, -1), offs=torch.tensor(ends, dtype=torch.int32))
    y.backward(dyc.float())
    return y.detach(), x.grad, w.grad


def test_function_against_the_restated_chain_and_the_reference_sqnr_bars():
    xc, wc, dyc = _inputs()
    y, gx, gw = _run(xc, wc, dyc, ENDS)
    # the offsets the backward drew: the same two draws from the same generator state
    torch.manual_seed(11)
    col_offset = int(torch.randint(0, 2 ** 32, (1,), dtype=torch.int64, device=_dev()))
    row_offset = int(torch.randint(0, 2 ** 32, (1,), dtype=torch.int64, device=_dev()))
    sums = restated_chain(xc, wc, dyc, ENDS, col_offset, row_offset)
    for e, (s, t) in enumerate(_slices(ENDS)):
        D._inside(f"out group {e}", y[s:t], *sums["out"][e], K)
        D._inside(f"grad_A group {e}", gx[s:t], *sums["grad_A"][e], N)
        D._inside(f"grad_B group {e}", gw[e], *sums["grad_B"][e], t - s)
    # the reference's own bars (test_nvfp4_grouped_mm.py); the restated chain alone has 16.76 / 15.07 / 15.62 dB on these inputs (CPU)
    for name, got, want, bar in zip(("out", "grad_A", "grad_B"), (y, gx, gw), fp32_grouped(xc, wc, dyc, ENDS), (15.0, 14.0, 12.0)):
        print(f"  SQNR {name}: {T.sqnr_db(got, want):.2f} dB (bar {bar})")
        assert T.sqnr_db(got, want) >= bar


def test_padding_equals_the_unpadded_call_on_padded_inputs():
    from ao_amd import ops

    xc, wc, dyc = _inputs()
    ends = [40, 40, 150, 256]  # groups that are no multiples of 16, one empty
    x_pad, starts, pad_ends = ops.fused_pad_token_groups(xc.to(_dev()), _offs(ends), 16)
    dy_pad = ops.fused_pad_token_groups(dyc.to(_dev()), _offs(ends), 16)[0]
    y, gx, gw = _run(xc, wc, dyc, ends, pad=True)
    yp, gxp, gwp = _run(x_pad.cpu(), wc, dy_pad.cpu(), pad_ends.cpu().tolist())
    unpad = lambda t: ops.fused_unpad_token_groups(t.to(_dev()), _offs(ends), starts, M, 16).cpu()  # noqa: E731
    assert torch.equal(R.bits(y), R.bits(unpad(yp))) and torch.equal(R.bits(gx), R.bits(unpad(gxp))) and torch.equal(R.bits(gw), R.bits(gwp))


def test_backward_replays_from_a_captured_graph():
    from ao_amd.prototype import _to_nvfp4_rht_rs_then_scaled_grouped_mm as grouped_mm

    xc, wc, dyc = _inputs()
    x, w, dy = xc.to(_dev()).requires_grad_(True), wc.to(_dev()).requires_grad_(True), dyc.to(_dev())
    seed, offs = D._i64(SEED), _offs(ENDS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):  # (the second pass alone is kept: gradients accumulate)
            x.grad = w.grad = None
            grouped_mm(x, w, SIGN, seed, offs).backward(dy)
    torch.cuda.current_stream().wait_stream(side)
    eager = (x.grad.cpu(), w.grad.cpu())
    x.grad = w.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grouped_mm(x, w, SIGN, seed, offs).backward(dy)
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append((x.grad.cpu(), w.grad.cpu()))
        for name, got, want in zip(("grad_A", "grad_B"), replays[-1], eager):
            # two stochastic roundings of the same gradient through the same GEMMs: the 6 dB bar tells a replay that computed something else
            print(f"  replay against the eager pass, {name}: {T.sqnr_db(got, want):.2f} dB")
            assert bool(torch.isfinite(got.float()).all()) and T.sqnr_db(got, want) > 6.0
    assert not torch.equal(R.bits(replays[0][0]), R.bits(replays[1][0]))  # the generator is a side input of the graph: fresh offsets a replay
