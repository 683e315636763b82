"""NVFP4 linears on the GPU (e2m1 codes, 1 x 16 e4m3 block scales, fp32 per-tensor scales): the cast and the per-tensor amax against the
reference's recorded bytes and, exhaustively, against the restated cast; dequantize; every route case of both linears with exact-sum
inputs against the restated chains bit for bit; the reference's recorded weight-only outputs; one-hot operands; Gaussian inputs inside the
float64 interval; and the tensor subclass through quantize_ (tests/nvfp4_ref.py, tests/nvfp4_cases.py, tests/golden/nvfp4.npz)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _parity  # noqa: E402
import nvfp4_cases as nc  # noqa: E402
import nvfp4_ref as R  # noqa: E402
from _parity import Guarded, check  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nvfp4.npz"))
KINDS = ["wo", "dyn"]
FORMS = {1: "nvfp4_stream_kernel", 2: "nvfp4_tile_kernel"}


def _dev():
    return torch.device("cuda", 0)


def _gbf(name):
    return torch.from_numpy(GOLDEN[name].view(np.int16).copy()).view(torch.bfloat16).to(_dev())


def _gu8(name):
    return torch.from_numpy(GOLDEN[name].copy()).to(_dev())


def _gf32(name):
    return torch.from_numpy(np.asarray(GOLDEN[name], dtype=np.float32).copy()).reshape(()).to(_dev())


def _e4m3(t):
    return t.view(torch.float8_e4m3fn)


def _lib_route(kind, M, N, K):
    from ao_amd import _lib

    return nc.route(_lib.lib(), kind, M, N, K)


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


# ---- 1. the cast and the per-tensor amax ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "given", "dyn"])
@pytest.mark.parametrize("name", ["cast", "edge", "nonf"])
def test_cast_equals_the_reference_bytes(name, mode):
    from ao_amd import ops

    x = _gbf(f"{name}_x")
    if mode == "dyn":
        p = ops.nvfp4_amax_scale(x)
        assert p.view(torch.int32).item() == _gf32(f"{name}_dyn_p").view(torch.int32).item()
    else:
        p = None if mode == "none" else _gf32("given_p")
    q, s = ops.nvfp4_quantize(x, p)
    assert q.dtype == torch.uint8 and s.dtype == torch.float8_e4m3fn and q.is_contiguous() and s.is_contiguous()
    assert torch.equal(q, _gu8(f"{name}_{mode}_q")), "codes differ from the reference's"
    assert torch.equal(s.view(torch.uint8), _gu8(f"{name}_{mode}_s")), "block scales differ from the reference's"


@pytest.mark.parametrize("shape", [(1, 16), (3, 4096), (257, 1040), (1040, 2064)], ids=lambda s: "%dx%d" % s)
def test_amax_scale_equals_max_abs_over_2688_in_bits(shape):
    """(1040 x 2064: more 16-byte pieces than the grid has threads, so the grid-stride loop runs.)  The maximum sits at a seeded place,
    negative in every other shape; then one NaN makes the result NaN, as torch.max does."""
    from ao_amd import ops

    g = torch.Generator().manual_seed(shape[0] + shape[1])
    x = torch.randn(shape, generator=g).to(torch.bfloat16)
    i = int(torch.randint(0, x.numel(), (1,), generator=g))
    x.view(-1)[i] = 7.53125 if shape[0] % 2 else -7.53125
    want = torch.max(torch.abs(x)).to(torch.float32) / 2688.0
    got = ops.nvfp4_amax_scale(x.to(_dev()))
    assert got.dtype == torch.float32 and got.dim() == 0
    assert got.cpu().view(torch.int32).item() == want.view(torch.int32).item()
    assert torch.max(torch.abs(x)).item() == 7.53125  # the planted element is the maximum
    x.view(-1)[(i * 7 + 3) % x.numel()] = float("nan")
    want = torch.max(torch.abs(x)).to(torch.float32) / 2688.0
    got = ops.nvfp4_amax_scale(x.to(_dev()))
    assert torch.isnan(want) and got.cpu().view(torch.int32).item() == want.view(torch.int32).item()


def test_amax_scale_and_cast_are_capturable():
    """No host read: the amax, the cast that reads it through its pointer and the GEMM replay in a graph on new data."""
    from ao_amd import ops

    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 256, generator=g).to(torch.bfloat16).to(_dev())
    w = (torch.randn(32, 256, generator=g) * 0.1).to(torch.bfloat16).to(_dev())
    wq, ws = ops.nvfp4_quantize(w)
    static = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.nvfp4_linear(static, wq, ws, dynamic_per_tensor_scale=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.nvfp4_linear(static, wq, ws, dynamic_per_tensor_scale=True)
    x2 = (x * 3 + 1).to(torch.bfloat16)
    static.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(R.bits(y), R.bits(ops.nvfp4_linear(x2, wq, ws, dynamic_per_tensor_scale=True)))


@pytest.mark.parametrize("with_p", [False, True], ids=["nop", "p"])
def test_cast_exhaustive(with_p):
    """Every finite bf16 value beside a fixed first element, 15 a block, for several first elements: the block's amax is that element or
    the value itself, so every value meets every kind of scale -- floor, normal, rounded, saturated."""
    from ao_amd import ops

    allbits = torch.arange(65536, dtype=torch.int32)
    finite = allbits[(allbits & 0x7F80) != 0x7F80].to(torch.int16).view(torch.bfloat16)
    assert finite.numel() == 65280 and finite.numel() % 15 == 0
    p = torch.tensor(0.0123, dtype=torch.float32) if with_p else None
    for amax in (6.0, 0.37109375, 2688.0, 1.0e-3, 30080.0, 2.0 ** -100):
        x = torch.cat([torch.full((finite.numel() // 15, 1), amax).to(torch.bfloat16), finite.reshape(-1, 15)], dim=1).contiguous()
        want_q, want_s = R.cast(x, p)
        q, s = ops.nvfp4_quantize(x.to(_dev()), None if p is None else p.to(_dev()))
        bad = (q.cpu() != want_q).any(dim=1) | (s.view(torch.uint8).cpu() != want_s).any(dim=1)
        assert not bool(bad.any()), "amax %r: %d blocks differ, first block %d: %r" % (
            amax, int(bad.sum()), int(torch.nonzero(bad)[0]), x[int(torch.nonzero(bad)[0])].tolist())


# ---- 2. dequantize --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "given"])
def test_dequantize_equals_the_reference_bits(mode):
    from ao_amd.prototype import NVFP4Tensor

    p = None if mode == "none" else _gf32("given_p")
    t = NVFP4Tensor.to_nvfp4(_gbf("cast_x"), per_tensor_scale=p)
    assert torch.equal(t.qdata, _gu8(f"cast_{mode}_q")) and t.is_swizzled_scales is False and tuple(t.scale.shape) == (12, 4)
    assert torch.equal(R.bits(t.dequantize()), R.bits(_gbf(f"deq_{mode}")))
    assert torch.equal(R.bits(t.t().dequantize().t().contiguous()), R.bits(_gbf(f"deq_{mode}")))


# ---- 3. exact sums, every route case ------------------------------------------------------------------------------------------------------
def _scales(shape, values, gen):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=gen)].to(torch.float8_e4m3fn).view(torch.uint8)


def assert_exact(S, unit, what):
    """Every term is a multiple of `unit` (by construction of the operands, asserted by the callers on the operands) and the absolute
    terms of an output sum to at most 2^24 units: every partial sum, in any order, is an integer below 2^24 units -- exact in fp32."""
    assert float(S.max()) <= 2.0 ** 24 * unit, "%s: sum of |terms| %.6g exceeds 2^24 units of %g" % (what, float(S.max()), unit)


def exact_problem(kind, M, N, K, with_p, seed):
    """Weight-only: integer x, |x| <= 8; any e2m1 codes; block scales in {1/4, 1/2, 1, 2}; a power-of-two per-tensor scale: terms are
    multiples of 2^-3 p with |term| <= 96 p.  Codes x codes: A scales in {1, 2}, B scales in {1/4, 1/2, 1, 2}, any positive fp32 pa, pb
    (applied after the sum): terms are multiples of 2^-4, |term| <= 144.  The bias is any bf16."""
    assert K <= 4096
    g = torch.Generator(device="cpu").manual_seed(seed)
    d = _dev()
    b = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
    b_s = _scales((N, K // 16), [0.25, 0.5, 1.0, 2.0], g)
    bias = (torch.randn(N, generator=g) * 3).to(torch.bfloat16)
    if kind == "wo":
        x = torch.randint(-8, 9, (M, K), generator=g).to(torch.bfloat16)
        pb = torch.tensor(2.0 ** (seed % 5 - 3), dtype=torch.float32) if with_p else None
        unit = 2.0 ** -3 * (float(pb) if with_p else 1.0)
        w = R.dequantize(b, b_s, pb).double()
        assert torch.equal(x.double(), x.double().round()) and torch.equal(w / unit, (w / unit).round())
        assert_exact(x.double().abs() @ w.abs().t(), unit, "weight-only")
        return dict(x=x.to(d), b=b.to(d), b_s=b_s.to(d), pb=None if pb is None else pb.to(d), bias=bias.to(d))
    a = torch.randint(0, 256, (M, K // 2), generator=g).to(torch.uint8)
    a_s = _scales((M, K // 16), [1.0, 2.0], g)
    pa = (torch.rand((), generator=g) * 0.02 + 1e-3).to(torch.float32) if with_p else None
    pb = (torch.rand((), generator=g) * 0.5 + 0.01).to(torch.float32) if with_p and seed % 3 else None
    ad, bd = R.dequantize(a, a_s, None, torch.float64), R.dequantize(b, b_s, None, torch.float64)
    assert torch.equal(ad * 2, (ad * 2).round()) and torch.equal(bd * 8, (bd * 8).round())
    assert_exact(ad.abs() @ bd.abs().t(), 2.0 ** -4, "codes x codes")
    return dict(a=a.to(d), a_s=a_s.to(d), b=b.to(d), b_s=b_s.to(d), pa=None if pa is None else pa.to(d), pb=None if pb is None else pb.to(d),
                bias=bias.to(d))


def run_problem(kind, pr, bias, buf):
    from ao_amd import ops

    if kind == "wo":
        ops.nvfp4_wo_linear(pr["x"], pr["b"], _e4m3(pr["b_s"]), pr["pb"], bias, out=buf.out)
        return R.wo_linear(pr["x"], pr["b"], pr["b_s"], pr["pb"], bias)
    ops.nvfp4_mm(pr["a"], _e4m3(pr["a_s"]), pr["b"], _e4m3(pr["b_s"]), pr["pa"], pr["pb"], bias, out=buf.out)
    return R.mm(pr["a"], pr["a_s"], pr["b"], pr["b_s"], pr["pa"], pr["pb"], bias)


def run_exact(kind, M, N, K, with_bias, with_p, seed):
    pr = exact_problem(kind, M, N, K, with_p, seed)
    buf = Guarded(M, N, torch.bfloat16, _dev())
    ref = run_problem(kind, pr, pr["bias"] if with_bias else None, buf)
    torch.cuda.synchronize()
    check(buf, ref_bits=R.bits(ref), route=_lib_route(kind, M, N, K))


@pytest.mark.parametrize("with_p", [False, True], ids=["nop", "p"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("idx", range(len(nc.CASES)), ids=["%s-%dx%dx%d" % c for c in nc.CASES])
def test_exact_every_route_case(idx, with_bias, with_p):
    kind, M, N, K = nc.CASES[idx]
    run_exact(kind, M, N, K, with_bias, with_p, seed=idx)


@pytest.mark.parametrize("shape", [(129, 1040, 528), (257, 1000, 144), (33, 1040, 2064), (16, 1000, 4096)],
                         ids=["tile-129x1040x528", "tile-257x1000x144", "stream-33x1040x2064", "stream-16x1000x4096"])
@pytest.mark.parametrize("kind", KINDS)
def test_exact_many_column_tiles(kind, shape):
    """The derivation picks the cheapest shape per requirement, so its wide cases have few k steps: here many column tiles WITH several
    k steps and a partial last one (K = 528, 144, 2064: a last block that stands alone), both forms."""
    M, N, K = shape
    assert _lib_route(kind, M, N, K)["kernel"] == ("tile" if M > 64 else "stream")
    run_exact(kind, M, N, K, True, True, seed=200 + M)


# ---- 4. the reference's recorded weight-only outputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [1, 2], ids=["stream", "tile"])
@pytest.mark.parametrize("tag", ["nop", "p"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
def test_golden_weight_only_outputs_bit_for_bit(tag, with_bias, form):
    from ao_amd import ops

    x, q, s = _gbf("lin_x"), _gu8("lin_q"), _e4m3(_gu8("lin_s"))
    buf = Guarded(x.shape[0], q.shape[0], torch.bfloat16, _dev())
    with forced_form(form):
        ops.nvfp4_wo_linear(x, q, s, _gf32("lin_p") if tag == "p" else None, _gbf("lin_bias") if with_bias else None, out=buf.out)
    check(buf, ref_bits=R.bits(_gbf(f"lin_{tag}_y" if with_bias else f"lin_{tag}_y_nobias")))


# ---- 5. one-hot operands ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [1, 2], ids=["stream", "tile"])
@pytest.mark.parametrize("with_p", [False, True], ids=["nop", "p"])
def test_one_hot_rows_return_dequantize(form, with_p):
    """80 one-hot rows (two grid rows of the forced stream form, two row tiles of the tiled form) over K = 272 (a last block that stands
    alone): the first k, the last k, a mid-block k and a spread of the others return dequantize()'s bits -- the per-element rounding of
    the weight under a per-tensor scale that is no power of two.  (A -0.0 weight returns +0.0: the accumulator starts at +0.0.)"""
    from ao_amd import ops
    from ao_amd.prototype import NVFP4Tensor

    torch.manual_seed(11)
    N, K, M = 40, 272, 80
    w = (torch.randn(N, K, device=_dev()) * torch.rand(N, 1, device=_dev()) * 3).to(torch.bfloat16)
    t = NVFP4Tensor.to_nvfp4(w, per_tensor_scale=ops.nvfp4_amax_scale(w) if with_p else None)
    ks = torch.tensor([0, K - 1, 77] + [(r * 37 + 5) % K for r in range(3, M)], device=_dev())
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=_dev())
    x[torch.arange(M, device=_dev()), ks] = 1
    want = (t.dequantize()[:, ks].t() + 0.0).contiguous()
    assert torch.equal(R.bits(t.dequantize()), R.bits(R.dequantize(t.qdata, t.scale.view(torch.uint8), t.per_tensor_scale)))
    assert len(set(R.unpack(t.qdata).reshape(-1).tolist())) == 16  # every code occurs
    buf = Guarded(M, N, torch.bfloat16, _dev())
    with forced_form(form):
        assert ops.nvfp4_linear_route(0, M, N, K)["kernel"] == FORMS[form]
        ops.nvfp4_wo_linear(x, t.qdata, t.scale, t.per_tensor_scale, out=buf.out)
    check(buf, ref_bits=R.bits(want))


@pytest.mark.parametrize("form", [1, 2], ids=["stream", "tile"])
def test_one_hot_codes_pin_the_lane_nibble_and_scale_map(form):
    """Codes x codes with ONE non-zero code (1.0) in each activation row, at a k that walks over every position of a block, every lane
    group and both forms' steps, under a block scale that differs from block to block: the output is that scale times the weight's
    dequantized column -- a wrong nibble, lane or scale byte on either side shows."""
    from ao_amd import ops

    g = torch.Generator().manual_seed(17)
    N, K, M = 40, 272, 80
    ks = torch.tensor([0, K - 1, 77] + [(r * 37 + 5) % K for r in range(3, M)])
    codes = torch.zeros(M, K, dtype=torch.uint8)
    codes[torch.arange(M), ks] = 2  # e2m1 1.0
    a = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    a_s = _scales((M, K // 16), [0.5, 1.0, 2.0, 4.0, 0.25], g)
    b = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
    b_s = _scales((N, K // 16), [0.25, 0.5, 1.0, 2.0, 1.5, 3.5, 0.4375], g)
    bd = R.dequantize(b, b_s, None, torch.float32)
    asel = a_s.view(torch.float8_e4m3fn).to(torch.float32)[torch.arange(M), ks // 16]
    want = ((bd[:, ks].t() * asel.reshape(M, 1)) + 0.0).to(torch.bfloat16)  # at most 2 + 4 + 1 significand bits: exact
    d = _dev()
    buf = Guarded(M, N, torch.bfloat16, d)
    with forced_form(form):
        assert ops.nvfp4_linear_route(1, M, N, K)["kernel"] == FORMS[form]
        ops.nvfp4_mm(a.to(d), _e4m3(a_s.to(d)), b.to(d), _e4m3(b_s.to(d)), out=buf.out)
    check(buf, ref_bits=R.bits(want.to(d)))
    assert torch.equal(R.bits(R.mm(a, a_s, b, b_s)), R.bits(want))


# ---- 6. Gaussian inputs ---------------------------------------------------------------------------------------------------------------------
def interval_problems(y, m64, S, K, chain):
    """y against the float64 sum m64: every element inside [chain(m64 - d), chain(m64 + d)], d = 2 K 2^-24 S (the accumulation allowance
    of _parity.bound; the chains are monotone: their scales are positive), and the fraction equal to chain(m64)."""
    d = 2.0 * K * 2.0 ** -24 * S
    lo, hi, mid = (chain(v).double() for v in (m64 - d, m64 + d, m64))
    yd = y.double()
    inside = (yd >= lo) & (yd <= hi)
    eq = (yd == mid).double().mean().item()
    print("%s: inside %.6f, equal %.6f" % (tuple(y.shape), inside.double().mean().item(), eq))
    msgs = []
    if not bool(inside.all()):
        i, j = (int(v) for v in torch.nonzero(~inside)[0])
        msgs.append("%d elements outside the interval, first at (%d, %d): %r not in [%r, %r]"
                    % (int((~inside).sum()), i, j, yd[i, j].item(), lo[i, j].item(), hi[i, j].item()))
    return msgs, eq


def gaussian_operands(shape):
    M, N, K = shape
    g = torch.Generator(device="cpu").manual_seed(M + N)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(_dev())
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(_dev())
    bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16).to(_dev())
    return x, w, bias


@pytest.mark.parametrize("form", [1, 2], ids=["stream", "tile"])
@pytest.mark.parametrize("shape", [(17, 1000, 4096), (33, 272, 1040)], ids=["17x1000x4096", "33x272x1040"])
@pytest.mark.parametrize("kind", KINDS)
def test_gaussian_inside_the_float64_interval(kind, shape, form):
    """Seeds as test_wo8_linear_gpu's.  A plain fp32 sequential accumulation of the same operands meets both conditions on the CPU
    (every element inside; equal fractions 0.9996 / 0.9997 weight-only, 1.0 / 1.0 codes x codes, whose chain rounds to bf16 three times)."""
    from ao_amd import ops

    M, N, K = shape
    x, w, bias = gaussian_operands(shape)
    pb = ops.nvfp4_amax_scale(w)
    b, b_s = ops.nvfp4_quantize(w, pb)
    buf = Guarded(M, N, torch.bfloat16, _dev())
    if kind == "wo":
        with forced_form(form):
            ops.nvfp4_wo_linear(x, b, b_s, pb, bias, out=buf.out)
        m64, S = R.wo_sums(x, b, b_s.view(torch.uint8), pb)
        chain = lambda v: R.wo_chain(v, bias)  # noqa: E731
    else:
        pa = ops.nvfp4_amax_scale(x)
        a, a_s = ops.nvfp4_quantize(x, pa)
        with forced_form(form):
            ops.nvfp4_mm(a, a_s, b, b_s, pa, pb, bias, out=buf.out)
        m64, S = R.mm_sums(a, a_s.view(torch.uint8), b, b_s.view(torch.uint8))
        chain = lambda v: R.mm_chain(v, pa, pb, bias)  # noqa: E731
    msgs, eq = interval_problems(buf.out, m64, S, K, chain)
    msgs = buf.guard_problems() + msgs
    if bool((buf.bits() == buf.sentinel).any()):
        msgs.append("elements left unwritten")
    assert not msgs, "; ".join(msgs)
    assert eq >= _parity.EQUAL_FRACTION, f"only {eq:.4f} of the elements equal chain(m64)"


# ---- 7. quantize_ ---------------------------------------------------------------------------------------------------------------------------
def exact_matrix(rows, k, gen, spread):
    """bf16 [rows, k] that the NVFP4 cast reproduces exactly, under a per-tensor scale that is a power of two: e2m1 values times
    448 2^-i 2^-12 per block (i <= spread), every block holding a 6, the first block i = 0 -- so max|w| = 2688 2^-12, p = 2^-12 and the
    block scales are 448 2^-i."""
    vals = torch.tensor(R.E2M1_VALUES, dtype=torch.float32)
    c = vals[torch.randint(0, 16, (rows, k // 16, 16), generator=gen)]
    c[:, :, 3] = 6.0
    i = torch.randint(0, spread + 1, (rows, k // 16, 1), generator=gen).to(torch.float32)
    i[0, 0, 0] = 0
    w = (c * 448.0 * torch.exp2(-i - 12)).reshape(rows, k)
    assert torch.equal(w, w.to(torch.bfloat16).to(torch.float32))
    return w.to(torch.bfloat16)


def _mlp(seed):
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Linear(128, 48, bias=True), torch.nn.ReLU(), torch.nn.Linear(48, 32, bias=False))
    model = model.to(torch.bfloat16).to(_dev())
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        model[0].weight.copy_(exact_matrix(48, 128, g, 2).to(_dev()))
        model[2].weight.copy_(exact_matrix(32, 48, g, 2).to(_dev()))
    return model


def _assert_bits(got, want):
    got = got.reshape(-1, got.shape[-1])
    bad = R.bits(got) != R.bits(want)
    assert not bool(bad.any()), "%d elements differ from nvfp4_ref, first at %r" % (int(bad.sum()), tuple(int(v) for v in torch.nonzero(bad)[0]))


@pytest.mark.parametrize("dynamic", [False, True], ids=["weight-only", "dynamic"])
def test_quantize_and_linear(dynamic):
    from ao_amd.prototype import (NVFP4DynamicActivationNVFP4WeightConfig, NVFP4Tensor, NVFP4WeightOnlyConfig,
                                  QuantizeTensorToNVFP4Kwargs)
    from ao_amd.quantization import quantize_

    model = _mlp(3)
    w0 = model[0].weight.detach().clone()
    quantize_(model, NVFP4DynamicActivationNVFP4WeightConfig() if dynamic else NVFP4WeightOnlyConfig())
    for lin, shape in ((model[0], (48, 128)), (model[2], (32, 48))):
        w = lin.weight
        assert isinstance(w, NVFP4Tensor) and isinstance(w, torch.nn.Parameter) and not w.requires_grad
        assert tuple(w.shape) == shape and tuple(w.qdata.shape) == (shape[0], shape[1] // 2) and tuple(w.scale.shape) == (shape[0], shape[1] // 16)
        assert w.is_swizzled_scales is False and w.block_size == 16 and w.orig_dtype == torch.bfloat16 and w.dtype == torch.bfloat16
        assert w.per_tensor_scale.dtype == torch.float32 and w.per_tensor_scale.dim() == 0 and w.per_tensor_scale.item() == 2.0 ** -12
        if dynamic:
            assert w.act_quant_kwargs == QuantizeTensorToNVFP4Kwargs(use_dynamic_per_tensor_scale=True, use_triton_kernel=True)
            assert w.use_triton_kernel is True
        else:
            assert w.act_quant_kwargs is None
    w = model[0].weight
    assert torch.equal(R.bits(w.dequantize()), R.bits(w0)), "the exact weight went through the cast unchanged"
    wq, ws, pw, bias = w.qdata, w.scale.view(torch.uint8), w.per_tensor_scale, model[0].bias
    g = torch.Generator().manual_seed(4)
    if dynamic:  # an activation the cast reproduces too: max|x| = 2688 2^-12 2^8, pa = 2^-4
        x = (exact_matrix(6, 128, g, 1).float() * 256).to(torch.bfloat16).reshape(2, 3, 128).to(_dev())
        a, a_s = R.cast(x.reshape(-1, 128).cpu(), R.amax_scale(x.cpu()))
        assert R.amax_scale(x.cpu()).item() == 2.0 ** -4
        ad, bd = R.dequantize(a, a_s, None, torch.float64), R.dequantize(wq.cpu(), ws.cpu(), None, torch.float64)
        assert torch.equal(ad * 2.0 ** -4, x.reshape(-1, 128).cpu().double()), "the exact activation goes through the cast unchanged"
        unit = (448 * 0.5 * 2.0 ** -1) * (448 * 0.5 * 2.0 ** -2)
        assert torch.equal(ad.reshape(-1, 1) * bd.reshape(1, -1) / unit, (ad.reshape(-1, 1) * bd.reshape(1, -1) / unit).round())
        assert_exact(ad.abs() @ bd.abs().t(), unit, "dynamic MLP layer")
        ref = lambda b: R.dynamic_linear(x.reshape(-1, 128).cpu(), wq.cpu(), ws.cpu(), pw.cpu(), dynamic=True, bias=b).to(_dev())  # noqa: E731
    else:
        x = torch.randint(-8, 9, (2, 3, 128), generator=g).to(torch.bfloat16).to(_dev())
        unit = 448 * 0.5 * 2.0 ** -14
        wd = w0.cpu().double()
        assert torch.equal(wd / unit, (wd / unit).round())
        assert_exact(x.reshape(-1, 128).cpu().double().abs() @ wd.abs().t(), unit, "weight-only MLP layer")
        ref = lambda b: R.wo_linear(x.reshape(-1, 128), wq, ws, pw, b)  # noqa: E731
    with torch.no_grad():
        y = model[0](x)
        y2 = F.linear(x, w)
        ym = torch.mm(x.reshape(-1, 128), w.t())
        ya = torch.addmm(bias, x.reshape(-1, 128), w.t())
        y0 = model[0](x[:0].reshape(0, 128))
        ys = F.linear(x, w[16:32], bias[16:32])
        full = model(x)
    assert y.shape == (2, 3, 48) and y.dtype == torch.bfloat16 and y0.shape == (0, 48) and full.shape == (2, 3, 32)
    _assert_bits(y, ref(bias.cpu() if dynamic else bias))
    _assert_bits(y2, ref(None))
    _assert_bits(ym, ref(None))
    _assert_bits(ya, ref(bias.cpu() if dynamic else bias))
    _assert_bits(ys, ref(bias.cpu() if dynamic else bias)[:, 16:32].contiguous())


def test_static_act_per_tensor_scale():
    """The static path: act_per_tensor_scale stored on the weight is the activation's per-tensor scale, whatever its amax."""
    from ao_amd.prototype import NVFP4Tensor, QuantizeTensorToNVFP4Kwargs

    g = torch.Generator().manual_seed(9)
    w = exact_matrix(48, 128, g, 2).to(_dev())
    x = (exact_matrix(5, 128, g, 1).float() * 256).to(torch.bfloat16).to(_dev())
    bias = (torch.randn(48, generator=g) * 3).to(torch.bfloat16).to(_dev())
    pw = torch.tensor(2.0 ** -12, device=_dev())
    for act_scale in (2.0 ** -4, 2.0 ** -3):  # the dynamic value and twice it: the block scales halve, still exact
        pa = torch.tensor(act_scale, device=_dev())
        t = NVFP4Tensor.to_nvfp4(w, per_tensor_scale=pw, act_per_tensor_scale=pa,
                                 act_quant_kwargs=QuantizeTensorToNVFP4Kwargs(use_dynamic_per_tensor_scale=False))
        assert t.act_per_tensor_scale is pa and torch.equal(R.bits(t.dequantize()), R.bits(w))
        with torch.no_grad():
            y = F.linear(x, t, bias)
        a, a_s = R.cast(x.cpu(), pa.cpu())
        assert torch.equal(R.dequantize(a, a_s, pa.cpu(), torch.float64), x.cpu().double())
        want = R.dynamic_linear(x.cpu(), t.qdata.cpu(), t.scale.view(torch.uint8).cpu(), pw.cpu(), pa=pa.cpu(), bias=bias.cpu())
        _assert_bits(y, want.to(_dev()))
    tn = NVFP4Tensor.to_nvfp4(w, act_quant_kwargs=QuantizeTensorToNVFP4Kwargs())  # neither per-tensor scale: one rounding, bias inside
    with torch.no_grad():
        y = F.linear(x, tn, bias)
    _assert_bits(y, R.dynamic_linear(x.cpu(), tn.qdata.cpu(), tn.scale.view(torch.uint8).cpu(), bias=bias.cpu()).to(_dev()))


@pytest.mark.parametrize("dynamic", [False, True], ids=["weight-only", "dynamic"])
def test_compiled_equals_eager(dynamic):
    from ao_amd.prototype import NVFP4DynamicActivationNVFP4WeightConfig, NVFP4WeightOnlyConfig
    from ao_amd.quantization import quantize_

    model = _mlp(6)
    quantize_(model, NVFP4DynamicActivationNVFP4WeightConfig() if dynamic else NVFP4WeightOnlyConfig())
    x = torch.randn(5, 128, dtype=torch.bfloat16, device=_dev())
    with torch.no_grad():
        eager = model(x)
        compiled = torch.compile(model, backend="aot_eager", fullgraph=True)(x)
    assert torch.equal(R.bits(eager), R.bits(compiled))
