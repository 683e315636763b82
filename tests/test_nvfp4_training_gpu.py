"""NVFP4 training on the GPU: the three casts against the reference's recorded bytes (tests/golden/nvfp4_training.npz) and, byte for byte,
against the restatement (tests/nvfp4_train_ref.py) at one block, at shapes ragged against the 128 x 128 tile in both directions and at
whole tiles, round to nearest even and stochastic rounding, fused and one direction at a time, inside guarded buffers; the scaled_mm
epilogue on both forms of the GEMM; and NVFP4Linear forward and backward against the restated chain and the recorded SQNR, through
quantize_, a state_dict, repeated backward passes and a captured graph.

Every case prints its figures before it asserts.  Measured on an MI355X (profiles/pytest_gpu_nvfp4_training.log): every cast byte-equal;
the Gaussian scaled_mm needs K >= 0 of 208 on both forms (every element within an ulp); the linear's worst |y - ref| / bound is 0.50 on
all three outputs at both shapes, SQNR out / grad_input / grad_weight 16.49 / 15.14 / 15.10 dB at (144, 80, 48) and 16.70 / 15.19 /
15.63 dB at (256, 128, 128), the restatement's to 0.01 dB; a graph replay is 14.3 - 14.7 dB from the eager pass."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _parity  # noqa: E402
import nvfp4_ref as R  # noqa: E402
import nvfp4_train_ref as T  # noqa: E402
from _parity import Guarded, check  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nvfp4_training.npz"))
SIGN = T.DEFAULT_SIGN_VECTOR
SHAPES = [(16, 16), (144, 80), (272, 144), (256, 128)]
SR_PAIRS = [(0x0123456789ABCDEF, 7), (-5, 2 ** 32 - 1)]
POISON = 0xA5


def _dev():
    return torch.device("cuda", 0)


def _gbf(name):
    return torch.from_numpy(GOLDEN[name].view(np.int16).copy()).view(torch.bfloat16)


def _gu8(name):
    return torch.from_numpy(GOLDEN[name].copy())


def _i64(v):
    v = int(v) & (2 ** 64 - 1)
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v], dtype=torch.int64, device=_dev())


class GuardedBytes:
    """_parity.Guarded's pattern for a uint8 output [rows, cols]: 256 poisoned bytes before it, 16 poisoned rows after it, the output
    16-byte aligned; `clean` says whether the guards still hold the poison."""

    def __init__(self, rows, cols):
        self.n = rows * cols
        raw = torch.full((256 + (rows + 16) * cols + 16,), POISON, dtype=torch.uint8, device=_dev())
        off = (-raw.data_ptr()) % 16
        self.raw = raw[off:off + 256 + (rows + 16) * cols]
        self.out = self.raw[256:256 + self.n].view(rows, cols)
        assert self.out.data_ptr() % 16 == 0

    def clean(self):
        return bool((self.raw[:256] == POISON).all()) and bool((self.raw[256 + self.n:] == POISON).all())


def _pairs(m, n):
    """guarded (codes, scales) for a cast of [m, n]"""
    return GuardedBytes(m, n // 2), GuardedBytes(m, n // 16)


def _row_col(x, amax2, sr=None, want_col=True, want_row=True):
    """the fused cast into guarded buffers -> CPU tensors (col_q, col_s, row_q, row_s), None for a direction not wanted"""
    from ao_amd import ops

    m, n = x.shape
    col = _pairs(n, m) if want_col else None
    row = _pairs(m, n) if want_row else None
    seed, co, ro = (None, None, None) if sr is None else (_i64(sr[0]), _i64(sr[1]), _i64(sr[2]))
    ops.nvfp4_train_quantize_row_col(x, amax2, SIGN, seed, co, ro, want_col=want_col, want_row=want_row,
                                     col_out=None if col is None else (col[0].out, col[1].out),
                                     row_out=None if row is None else (row[0].out, row[1].out))
    torch.cuda.synchronize()
    for g in (col or ()) + (row or ()):
        assert g.clean(), "a write outside the output"
    return tuple(None if g is None else g.out.cpu() for g in ((col or (None, None)) + (row or (None, None))))


def _weight_2d(w, amax):
    from ao_amd import ops

    n, k = w.shape
    a, b = _pairs(n, k), _pairs(k, n)
    ops.nvfp4_train_quantize_weight_2d(w, amax, out=(a[0].out, a[1].out), out_t=(b[0].out, b[1].out))
    torch.cuda.synchronize()
    for g in a + b:
        assert g.clean(), "a write outside the output"
    return tuple(g.out.cpu() for g in a + b)


def _same(got, want, what):
    for tag, g, w in zip(("col_q", "col_s", "row_q", "row_s"), got, want):
        if g is None:
            continue
        bad = (g != w).nonzero()
        assert len(bad) == 0, f"{what}: {len(bad)} bytes of {tag} differ, first at {tuple(bad[0].tolist())}: {int(g[tuple(bad[0])]):#x} vs {int(w[tuple(bad[0])]):#x}"


# ---- 1. the casts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["act", "edge", "zero"])
def test_casts_equal_the_reference_bytes(name):
    from ao_amd import ops

    x = _gbf(f"{name}_x").to(_dev())
    amax2 = ops.nvfp4_train_amax(x, SIGN)
    assert torch.equal(amax2.cpu().view(torch.int32), torch.from_numpy(GOLDEN[f"{name}_amax2"].copy()).view(torch.int32))
    _same(_row_col(x, amax2), [_gu8(f"{name}_{t}") for t in ("col_q", "col_s", "row_q", "row_s")], name)
    _same(_weight_2d(x, amax2[1]), [_gu8(f"{name}_{t}") for t in ("w2d_q", "w2d_s", "w2dt_q", "w2dt_s")], name + " 16 x 16")


def test_weight_cast_equals_the_reference_bytes():
    from ao_amd import ops

    w = _gbf("w_x").to(_dev())
    amax = ops.nvfp4_train_amax(w, 0, want_rht=False)
    assert float(amax[0]) == 0.0 and amax[1].cpu().view(torch.int32).item() == torch.from_numpy(GOLDEN["w_amax"].copy()).view(torch.int32).item()
    _same(_weight_2d(w, amax[1]), [_gu8(f"w_{t}") for t in ("w2d_q", "w2d_s", "w2dt_q", "w2dt_s")], "w")


def _matrix(m, n, seed):
    """Gaussian values on per-run magnitudes 2^-6 .. 2^6 with zeros, -0.0 and a few large and tiny outliers inside a run: the Hadamard sums
    round, and the restatement rounds them in the kernel's order."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, n, generator=g) * torch.exp2(torch.randint(-6, 7, (m // 16, 1), generator=g).float()).repeat_interleave(16, dim=0)
    x[torch.rand(m, n, generator=g) < 0.02] = 0.0
    x[torch.rand(m, n, generator=g) < 0.01] *= -0.0
    x[torch.rand(m, n, generator=g) < 0.01] *= 2.0 ** -14
    x[0, 0] = 300.0
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("m,n", SHAPES)
def test_casts_equal_the_restatement(m, n):
    from ao_amd import ops

    xc = _matrix(m, n, 100 + m + n)
    x = xc.to(_dev())
    want_amax = T.amaxes(xc, SIGN)
    amax2 = ops.nvfp4_train_amax(x, SIGN)
    assert torch.equal(amax2.cpu().view(torch.int32), want_amax.view(torch.int32)), (amax2.cpu(), want_amax)
    no_rht = ops.nvfp4_train_amax(x, SIGN, want_rht=False).cpu()
    assert float(no_rht[0]) == 0.0 and torch.equal(no_rht[1], want_amax[1])
    # round to nearest even: fused, and one direction at a time
    want = T.quantize_row_col(xc, want_amax, SIGN)
    fused = _row_col(x, amax2)
    _same(fused, want, f"{m} x {n} RTNE")
    _same(_row_col(x, amax2, want_col=False), (None, None) + want[2:], "row only")
    _same(_row_col(x, amax2, want_row=False), want[:2] + (None, None), "column only")
    # stochastic rounding: the restatement's bytes for two (seed, offsets)
    for seed, off in SR_PAIRS:
        sr = (seed, off, off ^ 0x5A5A)
        want_sr = T.quantize_row_col(xc, want_amax, SIGN, *sr)
        got_sr = _row_col(x, amax2, sr)
        _same(got_sr, want_sr, f"{m} x {n} SR seed {seed:#x} offset {off}")
        assert torch.equal(got_sr[1], want[1]) and torch.equal(got_sr[3], want[3])  # the scales do not depend on the rounding
        _same(_row_col(x, amax2, sr, want_col=False), (None, None) + want_sr[2:], "SR row only")
        _same(_row_col(x, amax2, sr, want_row=False), want_sr[:2] + (None, None), "SR column only")
        if m * n >= 1024:
            assert not torch.equal(got_sr[0], fused[0]) and not torch.equal(got_sr[2], fused[2])
    # the 16 x 16 cast, both directions
    _same(_weight_2d(x, amax2[1]), T.quantize_weight_2d(xc, want_amax[1]), f"{m} x {n} 16 x 16")


# ---- 2. the GEMM under the scaled_mm epilogue ----------------------------------------------------------------------------------------------
class forced_form:
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from ao_amd import ops

        ops.nvfp4_set_form(self.form)

    def __exit__(self, *exc):
        from ao_amd import ops

        ops.nvfp4_set_form(0)
        return False


def _exact_operand(rows, k, g):
    """integer-grid codes (0, 1, 2, 3, 4, 6 and their negatives) under block scales in {1/4, 1/2, 1, 2}"""
    lut = torch.tensor([0, 2, 4, 5, 6, 7, 8, 10, 12, 13, 14, 15], dtype=torch.uint8)
    c = lut[torch.randint(0, 12, (rows, k), generator=g)]
    s = torch.exp2(torch.randint(-2, 2, (rows, k // 16), generator=g).float()).to(torch.float8_e4m3fn).view(torch.uint8)
    return T.pack(c), s


@pytest.mark.parametrize("form", [1, 2])
def test_scaled_mm_exact_sums_are_bit_identical(form):
    from ao_amd import ops

    m, n, k = 40, 72, 256
    assert k * 144 * 16 <= 2 ** 24  # terms are multiples of 1/16, |term| <= (6 x 2)^2: every partial sum is exact in fp32
    g = torch.Generator().manual_seed(5)
    a, a_s = _exact_operand(m, k, g)
    b, b_s = _exact_operand(n, k, g)
    pa, pb = torch.tensor(2.0 ** -7), torch.tensor(2.0 ** 3)
    want = T.scaled_mm(a, a_s, b, b_s, pa, pb)
    buf = Guarded(m, n, torch.bfloat16, _dev())
    with forced_form(form):
        ops.nvfp4_scaled_mm(a.to(_dev()), a_s.to(_dev()), b.to(_dev()), b_s.to(_dev()), pa.to(_dev()), pb.to(_dev()), out=buf.out)
    torch.cuda.synchronize()
    check(buf, ref_bits=R.bits(want).to(_dev()))


@pytest.mark.parametrize("form", [1, 2])
def test_scaled_mm_gaussian_inside_the_float64_bound(form):
    from ao_amd import ops

    m, n, k = 100, 136, 208
    g = torch.Generator().manual_seed(6)
    xa, xb = torch.randn(m, k, generator=g).to(torch.bfloat16), (torch.randn(n, k, generator=g) * 0.1).to(torch.bfloat16)
    aa, ab = xa.float().abs().max(), xb.float().abs().max()
    a, a_s = T.cast(xa, aa)
    b, b_s = T.cast(xb, ab)
    pa, pb = T.amax_to_scale(aa), T.amax_to_scale(ab)   # not powers of two: the product of the scales rounds
    ref64, S = T.scaled_mm_sums(a, a_s, b, b_s, pa, pb)
    buf = Guarded(m, n, torch.bfloat16, _dev())
    with forced_form(form):
        ops.nvfp4_scaled_mm(a.to(_dev()), a_s.to(_dev()), b.to(_dev()), b_s.to(_dev()), pa.to(_dev()), pb.to(_dev()), out=buf.out)
    torch.cuda.synchronize()
    print(f"scaled_mm form {form}: the worst element needs K >= {_parity.k_needed(buf.out, ref64.to(_dev()), S.to(_dev()), torch.bfloat16):.1f} of {k}")
    check(buf, ref64=ref64.to(_dev()), S=S.to(_dev()), K=k)


def test_nvfp4_mm_keeps_its_own_chain():
    """ops.nvfp4_mm rounds the accumulator and P to bf16 first (the inference chain): the new epilogue flag leaves it as it was."""
    from ao_amd import ops

    m, n, k = 40, 72, 256
    g = torch.Generator().manual_seed(7)
    a, a_s = _exact_operand(m, k, g)
    b, b_s = _exact_operand(n, k, g)
    pa, pb = torch.tensor(0.0123), torch.tensor(1.7)
    bias = (torch.randn(n, generator=g)).to(torch.bfloat16)
    want = R.mm(a, a_s, b, b_s, pa, pb, bias)
    one = T.scaled_mm(a, a_s, b, b_s, pa, pb)
    assert not torch.equal(R.bits(R.mm(a, a_s, b, b_s, pa, pb)), R.bits(one))  # the two chains do differ on this input
    for form in (1, 2):
        buf = Guarded(m, n, torch.bfloat16, _dev())
        with forced_form(form):
            ops.nvfp4_mm(a.to(_dev()), a_s.to(_dev()), b.to(_dev()), b_s.to(_dev()), pa.to(_dev()), pb.to(_dev()), bias.to(_dev()), out=buf.out)
        torch.cuda.synchronize()
        check(buf, ref_bits=R.bits(want).to(_dev()))


# ---- 3. the linear ---------------------------------------------------------------------------------------------------------------------------
def _inside(name, y, ref64, S, K, bias=None):
    """|y - ref64| <= _parity.bound, printed before it is asserted.  With a bias, y = bf16(bf16(acc P) + bias): the GEMM's bound at ref64,
    where its rounding happens, plus half an ulp of a sum that may lie one binade above ref64 + bias -- one ulp at ref64 + bias."""
    b = _parity.bound(ref64, S, K, torch.bfloat16)
    if bias is not None:
        ref64 = ref64 + bias
        b = b + _parity.ulp(ref64, torch.bfloat16)
    err = (y.detach().double().cpu() - ref64).abs()
    worst = float((err / b).max())
    print(f"  {name}: worst |y - ref| / bound = {worst:.3f}, equal to the oracle's rounding: {float((y.cpu() == ref64.float().to(torch.bfloat16)).double().mean()):.4f}")
    assert bool((err <= b).all()), f"{name}: {int((err > b).sum())} elements outside the float64 bound, worst {worst:.2f} x"


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("name", ["lin0", "lin1"])
def test_linear_forward_backward_against_the_restated_chain(name, with_bias):
    from ao_amd.prototype import NVFP4Linear

    xc, wc, dyc, bc = _gbf(f"{name}_x"), _gbf(f"{name}_w"), _gbf(f"{name}_dy"), _gbf(f"{name}_bias")
    (m, k), n = xc.shape, wc.shape[0]
    lin = NVFP4Linear(k, n, bias=with_bias, rht_sign_vector=SIGN, device=_dev(), dtype=torch.bfloat16)
    seed = int(GOLDEN["sr_seed"])
    with torch.no_grad():
        lin.weight.copy_(wc)
        lin._sr_seed.fill_(seed)
        if with_bias:
            lin.bias.copy_(bc)
    x = xc.to(_dev()).requires_grad_(True)
    dy = dyc.to(_dev())
    torch.manual_seed(11)
    y = lin(x)
    y.backward(dy)
    torch.cuda.synchronize()
    # the offsets the backward drew: the same two draws from the same generator state
    torch.manual_seed(11)
    col_offset = int(torch.randint(0, 2 ** 32, (1,), dtype=torch.int64, device=_dev()))
    row_offset = int(torch.randint(0, 2 ** 32, (1,), dtype=torch.int64, device=_dev()))
    sums = T.linear_sums(xc, wc, dyc, SIGN, seed, col_offset, row_offset)
    print(f"{name} (M, K, N) = ({m}, {k}, {n}), bias {with_bias}, offsets {col_offset} {row_offset}")
    ref64, S = sums["out"]
    if with_bias:
        _inside("out", y, ref64, S, k, bias=bc.double())
        assert torch.equal(lin.bias.grad, dy.sum(dim=0))
    else:
        _inside("out", y, ref64, S, k)
    _inside("grad_input", x.grad, *sums["grad_input"], n)
    _inside("grad_weight", lin.weight.grad, *sums["grad_weight"], m)
    # SQNR against the fp32 matmuls: the casts are byte-equal to the restatement's and only the GEMM's summation order differs, so each
    # figure is within 0.5 dB below the one the generator measured on the restatement
    want = T.fp32_linear(xc, wc, dyc)
    stored = GOLDEN[f"{name}_sqnr"]
    got = {"out": T.sqnr_db(y.cpu(), want["out"] + (bc.float() if with_bias else 0.0)), "grad_input": T.sqnr_db(x.grad.cpu(), want["grad_input"]),
           "grad_weight": T.sqnr_db(lin.weight.grad.cpu(), want["grad_weight"])}
    floors = {"out": stored[3] if with_bias else stored[0], "grad_input": stored[1], "grad_weight": stored[2]}
    for key in got:
        print(f"  SQNR {key}: {got[key]:.2f} dB (the restatement: {floors[key]:.2f} dB)")
    for key in got:
        assert got[key] >= floors[key] - 0.5, f"SQNR of {key}: {got[key]:.2f} dB, the restatement has {floors[key]:.2f} dB"


def _model(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.GELU(), torch.nn.Linear(96, 32, bias=False)).to(_dev()).to(torch.bfloat16)


def test_quantize_is_bit_equal_to_a_model_of_nvfp4_linears_and_trains():
    from ao_amd.prototype import NVFP4Linear, NVFP4TrainingConfig
    from ao_amd.quantization import quantize_

    sv = tuple(-s for s in SIGN)
    a, b = _model(3), _model(3)
    quantize_(a, NVFP4TrainingConfig(rht_sign_vector=sv))
    b[0], b[2] = NVFP4Linear.from_linear(b[0], rht_sign_vector=sv), NVFP4Linear.from_linear(b[2], rht_sign_vector=sv)
    for i in (0, 2):
        assert type(a[i]) is NVFP4Linear and a[i].rht_sign_vector == sv
        with torch.no_grad():
            b[i]._sr_seed.copy_(a[i]._sr_seed)
    x = torch.randn(48, 64, device=_dev(), dtype=torch.bfloat16)
    grads = []
    for model in (a, b):
        torch.manual_seed(21)
        xi = x.clone().requires_grad_(True)
        out = model(xi)
        out.float().pow(2).mean().backward()
        grads.append((out, xi.grad, model[0].weight.grad, model[0].bias.grad, model[2].weight.grad))
    for u, v in zip(*grads):
        assert torch.equal(R.bits(u), R.bits(v))
    # a forward, a backward and an optimizer step
    opt = torch.optim.SGD(a.parameters(), lr=0.1)
    before = a[0].weight.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, a[0].weight) and bool(torch.isfinite(a[0].weight.float()).all())
    # a state_dict round trip keeps the sign vector
    fresh = _model(4)
    quantize_(fresh, NVFP4TrainingConfig())
    fresh.load_state_dict(a.state_dict())
    assert fresh[0].rht_sign_vector == sv and fresh[2].rht_sign_vector == sv
    torch.manual_seed(22)
    y1 = a(x)
    torch.manual_seed(22)
    assert torch.equal(R.bits(fresh(x)), R.bits(y1))


def test_two_backward_passes_round_with_other_bits():
    from ao_amd.prototype import NVFP4Linear

    torch.manual_seed(5)
    lin = NVFP4Linear(64, 48, rht_sign_vector=SIGN, device=_dev(), dtype=torch.bfloat16)
    x = torch.randn(32, 64, device=_dev(), dtype=torch.bfloat16)
    dy = torch.randn(32, 48, device=_dev(), dtype=torch.bfloat16)
    outs, grads = [], []
    for _ in range(2):
        xi = x.clone().requires_grad_(True)
        y = lin(xi)
        y.backward(dy)
        outs.append(y.detach())
        grads.append(xi.grad)
    assert torch.equal(R.bits(outs[0]), R.bits(outs[1]))           # the forward is round to nearest even
    assert not torch.equal(R.bits(grads[0]), R.bits(grads[1]))     # the offsets advanced


def test_backward_replays_under_a_captured_graph():
    from ao_amd.prototype import NVFP4Linear

    torch.manual_seed(6)
    lin = NVFP4Linear(64, 48, bias=True, rht_sign_vector=SIGN, device=_dev(), dtype=torch.bfloat16)
    x = torch.randn(32, 64, device=_dev(), dtype=torch.bfloat16, requires_grad=True)
    dy = torch.randn(32, 48, device=_dev(), dtype=torch.bfloat16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):  # (the second pass alone is kept: gradients accumulate)
            x.grad = None
            lin(x).backward(dy)
    torch.cuda.current_stream().wait_stream(side)
    eager = x.grad.detach().clone()
    x.grad = None
    lin.weight.grad = None
    lin.bias.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = lin(x)
        y.backward(dy)
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append((x.grad.detach().clone(), lin.weight.grad.detach().clone()))
    for gi, gw in replays:
        assert bool(torch.isfinite(gi.float()).all()) and bool(torch.isfinite(gw.float()).all()) and float(gi.float().abs().max()) > 0
        # the same GEMM on two stochastic roundings of the same gradient: 14.3 - 14.7 dB from each other as measured (the committed
        # log); the 6 dB bar is a smoke check that tells a replay that computed something else
        print(f"  replay against the eager pass: {T.sqnr_db(gi.cpu(), eager.cpu()):.2f} dB")
        assert T.sqnr_db(gi.cpu(), eager.cpu()) > 6.0
    assert not torch.equal(R.bits(replays[0][0]), R.bits(replays[1][0]))  # the generator is a side input of the graph: fresh offsets a replay
