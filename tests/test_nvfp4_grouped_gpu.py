"""NVFP4 grouped GEMM for MoE experts on the GPU (ao_nvfp4_grouped_mm and the grouped cast / amax): exact-sum operands against the per-group
chains bit for bit under the product route and under each forced form, one-hot rows against dequantize, Gaussian operands inside the
float64 interval, the grouped cast and amax against the dense ones per group, the reference's recorded outputs, and the Python layer
(tests/nvfp4_grouped_ref.py, tests/golden/nvfp4_grouped.npz)."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _parity  # noqa: E402
import nvfp4_grouped_ref as G  # noqa: E402
import nvfp4_ref as R  # noqa: E402
from _parity import Guarded, check  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(HERE, "golden", "nvfp4_grouped.npz"))
with open(os.path.join(os.path.dirname(HERE), "include", "ao_mi355.h")) as fh:
    SEAM = int(re.search(r"#define AO_NVFP4_GROUPED_STREAM_MAX_ROWS (\d+)", fh.read()).group(1))
FORMS = {1: "nvfp4_grouped_stream_kernel", 2: "nvfp4_grouped_tile_kernel"}
KINDS = ["wo", "dyn"]
KIND_ID = {"wo": 0, "dyn": 1}

_E256 = [0] * 256
_E256[5], _E256[130], _E256[255] = 3, 17, 1
# (group sizes, N, K, tail rows that no group owns and no launch may write)
CASES = [
    ([1], 1, 16, 0),
    ([0, 1, 16, 17], 17, 48, 0),                  # K no multiple of 32
    ([15, 0, 33], 130, 528, 5),                   # a partial last 128-step, a last block that stands alone, tail rows
    ([2, 0, 0, 5, 1, 0, 3, 1], 48, 2064, 0),      # K steps that do not divide over the waves
    ([64, 1, 0], 40, 144, 3),
    ([0, 0, 40], 16, 384, 0),
    ([65, 64], 130, 272, 0),                      # the tile-row boundary of the 64-row form
    ([129, 0, 200], 100, 256, 0),
    (_E256, 16, 128, 0),                          # E = 256, three non-empty groups
]
IDS = ["g1", "g0-1-16-17", "g15-0-33+5", "g8x", "g64-1-0+3", "g0-0-40", "g65-64", "g129-0-200", "e256"]
FORCED = [3, 7, 8]  # a stream form that walks a 200-row group in several passes, a tile form that serves 1-row groups, 256 experts
# The (m-tiles, waves) instances of the stream form that no case above launches, with the form forced: mean group sizes of 2 / 17 / 33
# rows take 1 / 2 / 4 m-tiles; one column tile (N = 16) asks for the most waves, the K / 128 k steps cap them.  (case, pair)
STREAM_PAIRS = [(([3, 1], 16, 512, 0), (1, 4)), (([3, 1], 16, 1024, 0), (1, 8)), (([20, 14], 16, 128, 0), (2, 1)),
                (([20, 14], 16, 1024, 0), (2, 8)), (([20, 14], 16, 2048, 0), (2, 16)), (([40, 26], 16, 128, 0), (4, 1)),
                (([40, 26], 16, 512, 0), (4, 4)), (([40, 26], 16, 1024, 0), (4, 8))]
EXACT_CASES = CASES + [case for case, _ in STREAM_PAIRS]  # what exact_problem indexes


def _dev():
    return torch.device("cuda", 0)


def _e4m3(t):
    return t.view(torch.float8_e4m3fn)


def _gbf(name):
    return torch.from_numpy(GOLDEN[name].view(np.int16).copy()).view(torch.bfloat16).to(_dev())


def _gu8(name):
    return torch.from_numpy(GOLDEN[name].copy()).to(_dev())


def _gf32(name):
    return torch.from_numpy(np.asarray(GOLDEN[name], dtype=np.float32).copy()).to(_dev())


class forced_form:
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from ao_amd import ops

        ops.nvfp4_grouped_mm_set_form(self.form)

    def __exit__(self, *exc):
        from ao_amd import ops

        ops.nvfp4_grouped_mm_set_form(0)
        return False


def expected_kernel(sizes, tail):
    """The product route: the seam (read from the header) on the mean group size ceil(M_total / E), tail rows included."""
    m_total, e = sum(sizes) + tail, len(sizes)
    return FORMS[1] if (m_total + e - 1) // e <= SEAM else FORMS[2]


def launch(kind, pr, out):
    from ao_amd import ops

    if kind == "wo":
        return ops.nvfp4_grouped_mm(0, pr["x"], None, pr["b"], _e4m3(pr["b_s"]), pr["offs"], None, pr["pb"], out=out)
    return ops.nvfp4_grouped_mm(1, pr["a"], _e4m3(pr["a_s"]), pr["b"], _e4m3(pr["b_s"]), pr["offs"], pr["pa"], pr["pb"], out=out)


def reference(kind, pr, b=None, b_s=None):
    b, b_s = (pr["b"] if b is None else b), (pr["b_s"] if b_s is None else b_s)
    if kind == "wo":
        return G.wo_linear(pr["x"], b, b_s, pr["offs"], pr["pb"])
    return G.mm(pr["a"], pr["a_s"], b, b_s, pr["offs"], pr["pa"], pr["pb"])


def to_dev(pr):
    return {k: (v.to(_dev()) if isinstance(v, torch.Tensor) else v) for k, v in pr.items()}


# ---- 1. exact sums pin every index -----------------------------------------------------------------------------------------------------------
def _scales(shape, values, gen):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=gen)].to(torch.float8_e4m3fn).view(torch.uint8)


def assert_exact(S, unit, what):
    """Every term is a multiple of `unit` (by construction, asserted by the callers on the operands) and the absolute terms of an output
    sum to at most 2^24 units: every partial sum, in any order, is an integer below 2^24 units -- exact in fp32."""
    assert float(S.max()) <= 2.0 ** 24 * unit, "%s: sum of |terms| %.6g exceeds 2^24 units of %g" % (what, float(S.max()), unit)


@functools.lru_cache(maxsize=None)
def exact_problem(kind, idx):
    """The operand recipe of test_nvfp4_gpu.exact_problem per expert (CPU tensors, built once and left unchanged).  Weight-only: integer x,
    |x| <= 8; any e2m1 codes; block scales in {1/4, 1/2, 1, 2}; a power-of-two scale per expert: group e's terms are multiples of
    2^-3 pb[e], |term| <= 96 pb[e].  Codes x codes: A scales in {1, 2}, any positive fp32 pa[e], pb[e] (applied after the sum): terms are
    multiples of 2^-4, |term| <= 144.  Neighbouring experts get different scales."""
    sizes, N, K, tail = EXACT_CASES[idx]
    E, M = len(sizes), sum(sizes) + tail
    assert K <= 4096
    g = torch.Generator(device="cpu").manual_seed(1000 + idx)
    offs = G.offs_of(sizes)
    b = torch.randint(0, 256, (E, N, K // 2), generator=g).to(torch.uint8)
    b_s = _scales((E, N, K // 16), [0.25, 0.5, 1.0, 2.0], g)
    if kind == "wo":
        x = torch.randint(-8, 9, (M, K), generator=g).to(torch.bfloat16)
        pb = torch.exp2(((torch.arange(E) * 3 + idx) % 5 - 3).to(torch.float32))
        assert torch.equal(x.double(), x.double().round())
        for e, r0, r1 in G.groups(offs):
            unit = 2.0 ** -3 * float(pb[e])
            w = R.dequantize(b[e], b_s[e], pb[e]).double()
            assert torch.equal(w / unit, (w / unit).round())
            assert_exact(x[r0:r1].double().abs() @ w.abs().t(), unit, "weight-only group %d" % e)
        pr = dict(x=x, b=b, b_s=b_s, pb=pb, offs=offs)
    else:
        a = torch.randint(0, 256, (M, K // 2), generator=g).to(torch.uint8)
        a_s = _scales((M, K // 16), [1.0, 2.0], g)
        pa = (torch.rand(E, generator=g) * 0.02 + 1e-3).to(torch.float32)
        pb = (torch.rand(E, generator=g) * 0.5 + 0.01).to(torch.float32)
        ad = R.dequantize(a, a_s, None, torch.float64)
        assert torch.equal(ad * 2, (ad * 2).round())
        for e in range(E):
            bd = R.dequantize(b[e], b_s[e], None, torch.float64)
            assert torch.equal(bd * 8, (bd * 8).round())
        assert_exact(G.mm_sums(a, a_s, b, b_s, offs)[1], 2.0 ** -4, "codes x codes")
        pr = dict(a=a, a_s=a_s, b=b, b_s=b_s, pa=pa, pb=pb, offs=offs)
    assert E == 1 or bool((pr["pb"][1:] != pr["pb"][:-1]).all()), "neighbouring experts share a scale"
    ref = reference(kind, pr)
    # the outputs tell the experts apart: every group against its NEIGHBOUR's weight (scales kept) gives other bits
    if E > 1:
        wrong = reference(kind, pr, torch.roll(b, 1, 0), torch.roll(b_s, 1, 0))
        for e, r0, r1 in G.groups(offs):
            assert not torch.equal(R.bits(ref[r0:r1]), R.bits(wrong[r0:r1])), "group %d: the neighbouring expert gives the same outputs" % e
    return dict(pr=to_dev(pr), ref_bits=R.bits(ref).to(_dev()), rows=int(offs[-1]), M=M, N=N)


def run_exact(kind, idx):
    p = exact_problem(kind, idx)
    buf = Guarded(p["M"], p["N"], torch.bfloat16, _dev())
    launch(kind, p["pr"], buf.out)
    torch.cuda.synchronize()
    check(buf, ref_bits=p["ref_bits"], written_rows=p["rows"])
    first = buf.bits()[:p["rows"]].clone()
    buf.poison(_parity.SENTINEL2)  # a second launch into a re-poisoned buffer: the same bits, the tail rows untouched again
    launch(kind, p["pr"], buf.out)
    torch.cuda.synchronize()
    check(buf, ref_bits=p["ref_bits"], written_rows=p["rows"])
    assert torch.equal(first, buf.bits()[:p["rows"]])


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_under_the_product_route(kind, idx):
    from ao_amd import ops

    sizes, N, K, tail = CASES[idx]
    assert ops.nvfp4_grouped_mm_kernel_name(KIND_ID[kind], sum(sizes) + tail, N, K, len(sizes)) == expected_kernel(sizes, tail)
    run_exact(kind, idx)


@pytest.mark.parametrize("form", [1, 2], ids=["stream", "tile"])
@pytest.mark.parametrize("idx", FORCED, ids=[IDS[i] for i in FORCED])
@pytest.mark.parametrize("kind", KINDS)
def test_exact_with_each_form_forced(kind, idx, form):
    from ao_amd import ops

    sizes, N, K, tail = CASES[idx]
    with forced_form(form):
        assert ops.nvfp4_grouped_mm_kernel_name(KIND_ID[kind], sum(sizes) + tail, N, K, len(sizes)) == FORMS[form]
        run_exact(kind, idx)


@pytest.mark.parametrize("case,pair", STREAM_PAIRS, ids=["g%s-k%d" % ("-".join(map(str, c[0])), c[2]) for c, _ in STREAM_PAIRS])
@pytest.mark.parametrize("kind", KINDS)
def test_exact_on_the_remaining_stream_instances(kind, case, pair):
    from ao_amd import ops

    sizes, N, K, tail = case
    with forced_form(1):
        route = ops.nvfp4_grouped_mm_route(KIND_ID[kind], sum(sizes) + tail, N, K, len(sizes))
        assert (route["kernel"], route["m_tiles"], route["waves"]) == (FORMS[1],) + pair
        run_exact(kind, EXACT_CASES.index(case))


def test_m_total_zero_launches_nothing():
    from ao_amd import ops

    d = _dev()
    y = ops.nvfp4_grouped_mm(0, torch.zeros(0, 32, dtype=torch.bfloat16, device=d), None, torch.zeros(2, 5, 16, dtype=torch.uint8, device=d),
                             torch.zeros(2, 5, 2, dtype=torch.float8_e4m3fn, device=d), torch.zeros(2, dtype=torch.int32, device=d))
    assert y.shape == (0, 5)


def test_bad_offs_cannot_address_outside():
    """Bounds are clamped to [0, M_total] and a non-increasing pair is an empty group: offs (5, 3, 30000) on 68 rows gives rows 0..4 to
    expert 0, none to expert 1 and rows 3..67 (the end clamped) to expert 2.  Both windows hold rows 3 and 4, which either may write last:
    the rows outside the overlap are compared, and the guards."""
    from ao_amd import ops

    pr = dict(exact_problem("wo", 4)["pr"])
    M, N = exact_problem("wo", 4)["M"], exact_problem("wo", 4)["N"]
    for form in (1, 2):
        buf = Guarded(M, N, torch.bfloat16, _dev())
        bad = torch.tensor([5, 3, 30000], dtype=torch.int32, device=_dev())
        with forced_form(form):
            ops.nvfp4_grouped_mm(0, pr["x"], None, pr["b"], _e4m3(pr["b_s"]), bad, None, pr["pb"], out=buf.out)
        torch.cuda.synchronize()
        assert not buf.guard_problems()
        want0 = R.wo_linear(pr["x"][:3], pr["b"][0], pr["b_s"][0], pr["pb"][0])
        want2 = R.wo_linear(pr["x"][5:], pr["b"][2], pr["b_s"][2], pr["pb"][2])
        assert torch.equal(R.bits(buf.out[:3]), R.bits(want0)) and torch.equal(R.bits(buf.out[5:]), R.bits(want2))


# ---- 2. one-hot rows return dequantize ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [1, 2], ids=["stream", "tile"])
@pytest.mark.parametrize("with_p", [False, True], ids=["nop", "p"])
def test_one_hot_rows_return_dequantize(form, with_p):
    """test_nvfp4_gpu's construction per group: 80 one-hot rows in groups of 38 / 0 / 25 / 17 over K = 272 (a last block that stands alone),
    the first k, the last k, a mid-block k and a spread of the others, return the bits of THAT expert's dequantize() under per-expert
    scales that are no powers of two: the expert base, the nibble, the lane and the scale byte.  (A -0.0 weight returns +0.0.)"""
    from ao_amd import ops
    from ao_amd.prototype import NVFP4ExpertWeights

    torch.manual_seed(11)
    sizes, N, K = [38, 0, 25, 17], 40, 272
    E, M = len(sizes), sum(sizes)
    d = _dev()
    w = (torch.randn(E, N, K, device=d) * torch.rand(E, N, 1, device=d) * torch.tensor([3.0, 1.0, 0.11, 47.0], device=d).reshape(E, 1, 1))
    experts = NVFP4ExpertWeights.from_hp(w.to(torch.bfloat16), use_per_expert_scale=with_p)
    if with_p:
        frac = torch.frexp(experts.per_tensor_scale)[0]
        assert bool((frac != 0.5).all()) and len(set(experts.per_tensor_scale.tolist())) == E
    offs = G.offs_of(sizes, d)
    ks = torch.tensor([0, K - 1, 77] + [(r * 37 + 5) % K for r in range(3, M)], device=d)
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=d)
    x[torch.arange(M, device=d), ks] = 1
    deq = experts.dequantize()
    assert torch.equal(R.bits(deq), R.bits(G.dequantize(experts.qdata, experts.scale.view(torch.uint8), experts.per_tensor_scale)))
    want = torch.zeros(M, N, dtype=torch.bfloat16, device=d)
    for e, r0, r1 in G.groups(offs):
        want[r0:r1] = (deq[e][:, ks[r0:r1]].t() + 0.0)
        assert torch.equal(R.bits(experts[e].dequantize()), R.bits(deq[e]))
    buf = Guarded(M, N, torch.bfloat16, d)
    with forced_form(form):
        assert ops.nvfp4_grouped_mm_route(0, M, N, K, E)["kernel"] == FORMS[form]
        ops.nvfp4_grouped_mm(0, x, None, experts.qdata, experts.scale, offs, None, experts.per_tensor_scale, out=buf.out)
    check(buf, ref_bits=R.bits(want))


# ---- 3. Gaussian operands ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gaussian_problem(kind, idx):
    """CPU tensors: x ~ N(0, 1), w ~ 0.05 N(0, 1) times a per-expert factor, the weight cast under its per-expert amax scale and (codes x
    codes) the activation under its per-group amax scale, both by the CPU restatement -- the bytes the kernels' casts give."""
    sizes, N, K, tail = CASES[idx]
    E, M = len(sizes), sum(sizes) + tail
    g = torch.Generator(device="cpu").manual_seed(2000 + idx)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(E, N, K, generator=g) * 0.05 * torch.exp2((torch.arange(E) % 4).to(torch.float32)).reshape(E, 1, 1)).to(torch.bfloat16)
    offs = G.offs_of(sizes)
    woffs = G.offs_of([N] * E)
    pb = G.group_amax_scale(w.reshape(E * N, K), woffs)
    b, b_s = (t.reshape(E, N, -1) for t in G.cast(w.reshape(E * N, K), woffs, pb))
    if kind == "wo":
        return dict(x=x, b=b, b_s=b_s, pb=pb, offs=offs)
    pa = G.group_amax_scale(x, offs)
    a, a_s = G.cast(x, offs, pa)
    return dict(a=a, a_s=a_s, b=b, b_s=b_s, pa=pa, pb=pb, offs=offs)


def gaussian_sums(kind, pr):
    if kind == "wo":
        m64, S = G.wo_sums(pr["x"], pr["b"], pr["b_s"], pr["offs"], pr["pb"])
        return m64, S, R.wo_chain
    m64, S = G.mm_sums(pr["a"], pr["a_s"], pr["b"], pr["b_s"], pr["offs"])
    return m64, S, lambda v: G.mm_chain(v, pr["offs"], pr["pa"], pr["pb"])


def run_gaussian(kind, idx):
    sizes, N, K, tail = CASES[idx]
    pr = gaussian_problem(kind, idx)
    rows, M = int(pr["offs"][-1]), sum(sizes) + tail
    buf = Guarded(M, N, torch.bfloat16, _dev())
    launch(kind, to_dev(pr), buf.out)
    torch.cuda.synchronize()
    m64, S, chain = gaussian_sums(kind, pr)
    msgs, eq = G.interval_problems(buf.out[:rows].cpu(), m64[:rows], S[:rows], K, chain)
    msgs = buf.guard_problems() + msgs
    if bool((buf.bits()[:rows] == buf.sentinel).any()):
        msgs.append("elements left unwritten")
    if bool((buf.bits()[rows:] != buf.sentinel).any()):
        msgs.append("tail rows written")
    assert not msgs, "; ".join(msgs)
    if rows * N >= _parity.EQUAL_MIN_ELEMENTS:
        assert eq >= _parity.EQUAL_FRACTION, f"only {eq:.4f} of the elements equal chain(m64)"


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_gaussian_inside_the_float64_interval(kind, idx):
    """The dense NVFP4 tests' conditions: every output inside the float64 interval d = 2 K 2^-24 S under the chain and, on the cases with at
    least 1024 written elements, at least 0.97 of them equal to chain(m64).  A plain sequential fp32 accumulation of the same operands on
    the CPU meets both on every case: every element inside, and the equal fraction 1.0 on every case of both kinds but g65-64
    weight-only, 0.9999."""
    run_gaussian(kind, idx)


@pytest.mark.parametrize("form", [1, 2], ids=["stream", "tile"])
@pytest.mark.parametrize("idx", [2, 7], ids=[IDS[2], IDS[7]])
@pytest.mark.parametrize("kind", KINDS)
def test_gaussian_with_each_form_forced(kind, idx, form):
    with forced_form(form):
        run_gaussian(kind, idx)


# ---- 4. the grouped cast and amax ---------------------------------------------------------------------------------------------------------------
def _cast_operands():
    g = torch.Generator().manual_seed(7)
    sizes, K, tail = [5, 0, 17, 3], 80, 2
    M = sum(sizes) + tail
    x = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 7, (M, 1), generator=g).to(torch.float32))).to(torch.bfloat16)
    return sizes, x.to(_dev()), G.offs_of(sizes, _dev())


@pytest.mark.parametrize("with_nan", [False, True], ids=["finite", "nan"])
def test_grouped_amax_and_cast_equal_the_dense_ones_per_group(with_nan):
    from ao_amd import ops

    sizes, x, offs = _cast_operands()
    if with_nan:
        x[7, 33] = float("nan")  # in group 2
    rows = int(offs[-1])
    p = ops.nvfp4_group_amax_scale(x, offs)
    assert p.dtype == torch.float32 and tuple(p.shape) == (len(sizes),)
    q, s = ops.nvfp4_quantize_grouped(x, p, offs)
    assert q.dtype == torch.uint8 and s.dtype == torch.float8_e4m3fn and tuple(q.shape) == (x.shape[0], 40) and tuple(s.shape) == (x.shape[0], 5)
    qn, sn = ops.nvfp4_quantize_grouped(x, None, offs)
    for e, r0, r1 in G.groups(offs):
        pe = ops.nvfp4_amax_scale(x[r0:r1].contiguous())
        assert p[e].view(torch.int32).item() == pe.view(torch.int32).item(), "group %d: the scale's bits differ" % e
        qe, se = ops.nvfp4_quantize(x[r0:r1].contiguous(), pe)
        assert torch.equal(q[r0:r1], qe) and torch.equal(s[r0:r1].view(torch.uint8), se.view(torch.uint8)), "group %d" % e
    assert p[1].item() == 0.0 and bool(torch.isnan(p[2])) == with_nan
    qd, sd = ops.nvfp4_quantize(x[:rows].contiguous())
    assert torch.equal(qn[:rows], qd) and torch.equal(sn[:rows].view(torch.uint8), sd.view(torch.uint8))
    for t in (q, s.view(torch.uint8), qn, sn.view(torch.uint8)):
        assert not bool(t[rows:].any()), "rows past offs[-1] were written"
    # the CPU restatement gives the same bytes
    pc = G.group_amax_scale(x.cpu(), offs.cpu())
    assert torch.equal(pc.view(torch.int32), p.cpu().view(torch.int32))
    if not with_nan:
        qc, sc = G.cast(x.cpu(), offs.cpu(), pc)
        assert torch.equal(qc, q.cpu()) and torch.equal(sc, s.view(torch.uint8).cpu())


def test_group_amax_many_rows_and_experts():
    """More 16-byte pieces a group than one pass of its workgroups covers (the grid-stride loop runs), and 300 groups (two blocks of the
    clear and scale kernels)."""
    from ao_amd import ops

    g = torch.Generator().manual_seed(8)
    x = torch.randn(2100, 2064, generator=g).to(torch.bfloat16)
    sizes = [2000, 0, 100]
    x[1999, 2063] = -9.25
    x[2050, 0] = 11.5
    got = ops.nvfp4_group_amax_scale(x.to(_dev()), G.offs_of(sizes, _dev()))
    assert torch.equal(got.cpu().view(torch.int32), G.group_amax_scale(x, G.offs_of(sizes)).view(torch.int32))
    assert torch.equal(got.cpu(), torch.tensor([9.25, 0.0, 11.5], dtype=torch.float32) / 2688.0)
    sizes = [i % 3 for i in range(300)]
    x = torch.randn(sum(sizes), 32, generator=g).to(torch.bfloat16)
    got = ops.nvfp4_group_amax_scale(x.to(_dev()), G.offs_of(sizes, _dev()))
    assert torch.equal(got.cpu().view(torch.int32), G.group_amax_scale(x, G.offs_of(sizes)).view(torch.int32))


@pytest.mark.parametrize("tag", ["p", "nop"])
def test_from_hp_equals_the_reference_bytes(tag):
    from ao_amd.prototype import NVFP4ExpertWeights

    experts = NVFP4ExpertWeights.from_hp(_gbf("w3_w"), use_per_expert_scale=tag == "p")
    assert torch.equal(experts.qdata, _gu8(f"w3_{tag}_q")), "codes differ from the reference's"
    assert torch.equal(experts.scale.view(torch.uint8), _gu8(f"w3_{tag}_s")), "block scales differ from the reference's"
    if tag == "p":
        assert torch.equal(experts.per_tensor_scale.view(torch.int32), _gf32("w3_p").view(torch.int32))
    else:
        assert experts.per_tensor_scale is None
    assert torch.equal(R.bits(experts.dequantize()), R.bits(_gbf(f"w3_{tag}_deq")))


def test_grouped_amax_and_cast_are_capturable():
    """No host read: the per-group amax and the cast that reads it (and offs) through pointers replay in a graph on new data AND new
    group bounds."""
    from ao_amd import ops

    sizes, x, offs = _cast_operands()
    sx, so = x.clone(), offs.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.nvfp4_quantize_grouped(sx, ops.nvfp4_group_amax_scale(sx, so), so)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p = ops.nvfp4_group_amax_scale(sx, so)
        q, sc = ops.nvfp4_quantize_grouped(sx, p, so)
    x2 = (x * 3 + 1).to(torch.bfloat16)
    offs2 = G.offs_of([2, 9, 0, 14], _dev())
    sx.copy_(x2)
    so.copy_(offs2)
    q.zero_()
    sc.view(torch.uint8).zero_()
    graph.replay()
    torch.cuda.synchronize()
    p2 = ops.nvfp4_group_amax_scale(x2, offs2)
    q2, s2 = ops.nvfp4_quantize_grouped(x2, p2, offs2)
    assert torch.equal(p.view(torch.int32), p2.view(torch.int32)) and torch.equal(q, q2) and torch.equal(sc.view(torch.uint8), s2.view(torch.uint8))


# ---- 5. the reference's recorded outputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [1, 2], ids=["stream", "tile"])
@pytest.mark.parametrize("tag", ["p", "nop"])
def test_golden_weight_only_outputs_bit_for_bit(tag, form):
    """torch._grouped_mm(x, dequantize(bf16)^T, offs) as the reference computed it on exact-sum operands."""
    from ao_amd import ops

    x, q, s = _gbf("gw_x"), _gu8("gw_q"), _e4m3(_gu8("gw_s"))
    offs = G.offs_of(GOLDEN["gw_sizes"].tolist(), _dev())
    buf = Guarded(x.shape[0], q.shape[1], torch.bfloat16, _dev())
    with forced_form(form):
        ops.nvfp4_grouped_mm(0, x, None, q, s, offs, None, _gf32("gw_p") if tag == "p" else None, out=buf.out)
    check(buf, ref_bits=R.bits(_gbf(f"gw_{tag}_y")))


@pytest.mark.parametrize("form", [1, 2], ids=["stream", "tile"])
def test_golden_emulated_codes_outputs(form):
    """_emulated_nvfp4_scaled_grouped_mm_2d_3d's recorded output against the kernel's, both by their l2 distance to float64: the kernel's
    must not exceed the emulation's."""
    from ao_amd import ops

    a, a_s, b, b_s = _gu8("ge_aq"), _gu8("ge_as"), _gu8("gw_q"), _gu8("gw_s")
    offs = G.offs_of(GOLDEN["gw_sizes"].tolist(), _dev())
    buf = Guarded(a.shape[0], b.shape[1], torch.bfloat16, _dev())
    with forced_form(form):
        ops.nvfp4_grouped_mm(1, a, _e4m3(a_s), b, _e4m3(b_s), offs, out=buf.out)
    torch.cuda.synchronize()
    assert not buf.guard_problems() and not bool((buf.bits() == buf.sentinel).any())
    m64, _ = G.mm_sums(a.cpu(), a_s.cpu(), b.cpu(), b_s.cpu(), offs.cpu())
    kernel = float(torch.linalg.norm(buf.out.cpu().double() - m64))
    emulated = float(torch.linalg.norm(_gbf("ge_y").cpu().double() - m64))
    print("l2 to float64: kernel %.6g, emulation %.6g (|m64| %.6g)" % (kernel, emulated, float(torch.linalg.norm(m64))))
    assert kernel <= emulated


# ---- 6. the Python layer ---------------------------------------------------------------------------------------------------------------------------
def exact_matrix(rows, k, gen, spread):
    """(test_nvfp4_gpu.exact_matrix.)  bf16 [rows, k] that the NVFP4 cast reproduces exactly under a per-tensor scale that is a power of
    two: e2m1 values times 448 2^-i 2^-12 per block (i <= spread), every block holding a 6, the first block i = 0 -- so
    max|w| = 2688 2^-12, p = 2^-12 and the block scales are 448 2^-i."""
    vals = torch.tensor(R.E2M1_VALUES, dtype=torch.float32)
    c = vals[torch.randint(0, 16, (rows, k // 16, 16), generator=gen)]
    c[:, :, 3] = 6.0
    i = torch.randint(0, spread + 1, (rows, k // 16, 1), generator=gen).to(torch.float32)
    i[0, 0, 0] = 0
    w = (c * 448.0 * torch.exp2(-i - 12)).reshape(rows, k)
    assert torch.equal(w, w.to(torch.bfloat16).to(torch.float32))
    return w.to(torch.bfloat16)


def _python_problem():
    """Experts and activations the casts reproduce exactly, scaled by a power of two per expert / group so that the per-expert and
    per-group scales differ: p_e = 2^(e - 12), pa_e = 2^(e - 4)."""
    g = torch.Generator().manual_seed(21)
    sizes, N, K = [5, 0, 3, 7], 48, 128
    E = len(sizes)
    w = torch.stack([(exact_matrix(N, K, g, 2).float() * 2.0 ** e).to(torch.bfloat16) for e in range(E)])
    xs = [(exact_matrix(max(m, 1), K, g, 1).float() * 256 * 2.0 ** e).to(torch.bfloat16)[:m] for e, m in enumerate(sizes)]
    xi = torch.randint(-8, 9, (sum(sizes), K), generator=g).to(torch.bfloat16)
    return sizes, w.to(_dev()), torch.cat(xs).to(_dev()), xi.to(_dev())


def _assert_exact_products(A, B, ua, ub):
    """A [m, K], B [n, K] float64: entries multiples of ua / ub, and every output's absolute terms sum to at most 2^24 ua ub"""
    assert torch.equal(A / ua, (A / ua).round()) and torch.equal(B / ub, (B / ub).round())
    assert_exact(A.abs() @ B.abs().t(), ua * ub, "python-layer problem")


@pytest.mark.parametrize("mode", ["weight_only", "static", "dynamic"])
def test_python_grouped_mm_equals_the_dense_linears_per_group(mode):
    from ao_amd.prototype import NVFP4ExpertWeights, NVFP4Tensor, QuantizeTensorToNVFP4Kwargs, nvfp4_grouped_mm

    sizes, w, xd, xi = _python_problem()
    E = len(sizes)
    offs = G.offs_of(sizes, _dev())
    pa = torch.exp2(torch.arange(E, dtype=torch.float32) - 4).to(_dev())
    experts = NVFP4ExpertWeights.from_hp(w, act_per_tensor_scale=pa if mode == "static" else None)
    assert experts.per_tensor_scale.tolist() == [2.0 ** (e - 12) for e in range(E)]
    assert torch.equal(R.bits(experts.dequantize()), R.bits(w)), "the exact weights went through the cast unchanged"
    x = xi if mode == "weight_only" else xd
    for e, r0, r1 in G.groups(offs):
        wd = w[e].cpu().double()
        if mode == "weight_only":
            _assert_exact_products(x[r0:r1].cpu().double(), wd, 1.0, 448 * 0.5 * 2.0 ** (e - 14))
        else:
            _assert_exact_products(x[r0:r1].cpu().double(), wd, 448 * 0.5 * 2.0 ** (e - 5), 448 * 0.5 * 2.0 ** (e - 14))
            assert R.amax_scale(x[r0:r1].cpu()).item() == 2.0 ** (e - 4)
    y = nvfp4_grouped_mm(x, experts, offs, weight_only=mode == "weight_only", use_dynamic_per_group_scale=mode == "dynamic")
    assert y.shape == (sum(sizes), 48) and y.dtype == torch.bfloat16
    kw = None if mode == "weight_only" else QuantizeTensorToNVFP4Kwargs(use_dynamic_per_tensor_scale=mode == "dynamic")
    for e, r0, r1 in G.groups(offs):
        t = experts[e]
        assert isinstance(t, NVFP4Tensor) and t.per_tensor_scale.dim() == 0
        dense = NVFP4Tensor(t.qdata, t.scale, 16, torch.bfloat16, t.per_tensor_scale, t.act_per_tensor_scale, False, False, kw)
        with torch.no_grad():
            want = F.linear(x[r0:r1], dense)
        assert torch.equal(R.bits(y[r0:r1]), R.bits(want)), "group %d differs from the dense linear" % e
    with torch.no_grad():
        compiled = torch.compile(lambda a: nvfp4_grouped_mm(a, experts, offs, weight_only=mode == "weight_only",
                                                            use_dynamic_per_group_scale=mode == "dynamic"),
                                 backend="aot_eager", fullgraph=True)(x)
    assert torch.equal(R.bits(compiled), R.bits(y))


def test_from_nvfp4_tensors_stacks_the_dense_casts():
    from ao_amd import ops
    from ao_amd.prototype import NVFP4ExpertWeights, NVFP4Tensor

    _, w, _, _ = _python_problem()
    dense = [NVFP4Tensor.to_nvfp4(w[e].contiguous(), per_tensor_scale=ops.nvfp4_amax_scale(w[e].contiguous())) for e in range(w.shape[0])]
    a, b = NVFP4ExpertWeights.from_nvfp4_tensors(dense), NVFP4ExpertWeights.from_hp(w)
    assert torch.equal(a.qdata, b.qdata) and torch.equal(a.scale.view(torch.uint8), b.scale.view(torch.uint8))
    assert torch.equal(a.per_tensor_scale.view(torch.int32), b.per_tensor_scale.view(torch.int32))


def test_refusals_carry_the_reason():
    from ao_amd.prototype import NVFP4ExpertWeights, NVFP4Tensor, nvfp4_grouped_mm

    _, w, xd, _ = _python_problem()
    experts = NVFP4ExpertWeights.from_hp(w)
    offs = G.offs_of([5, 0, 3, 7], _dev())
    with pytest.raises(NotImplementedError, match="takes bfloat16 activations, got torch.float32"):
        nvfp4_grouped_mm(xd.float(), experts, offs)
    with pytest.raises(NotImplementedError, match="3-D.*NVFP4ExpertWeights"):
        NVFP4Tensor.to_nvfp4(w)
    with pytest.raises(NotImplementedError, match="per-expert.*NVFP4ExpertWeights"):
        NVFP4Tensor(experts.qdata[0], experts.scale[0], 16, torch.bfloat16, experts.per_tensor_scale.reshape(-1, 1, 1))
    with pytest.raises(RuntimeError, match="offs must be int32"):
        from ao_amd import ops

        ops.nvfp4_grouped_mm(0, xd, None, experts.qdata, experts.scale, offs.long())
