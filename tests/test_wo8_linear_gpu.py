"""int8 / float8 weight-only linears on the GPU (bf16 activation x 8-bit weight): every route case with exact-sum inputs against the
restated chain bit for bit, the reference's recorded outputs, one-hot activations, Gaussian inputs inside the float64 interval, and the
tensor subclasses through quantize_ (tests/wo8_ref.py, tests/wo8_cases.py, tests/golden/wo8.npz)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _parity  # noqa: E402
import wo8_cases as wc  # noqa: E402
import wo8_ref as R  # noqa: E402
from _parity import Guarded, check  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wo8.npz"))
FMT_NAMES = ["int8", "e4m3"]


def _dev():
    return torch.device("cuda", 0)


def _op(fmt):
    from ao_amd import ops

    return ops.int8_wo_linear if fmt == "int8" else ops.fp8_wo_linear


def _gbf(name):
    return torch.from_numpy(GOLDEN[name].view(np.int16).copy()).view(torch.bfloat16).to(_dev())


def _gcodes(fmt, name):
    q = torch.from_numpy(GOLDEN[name].copy()).to(_dev())
    return q if fmt == "int8" else q.view(torch.float8_e4m3fn)


def _lib_route(fmt, M, N, K):
    from ao_amd import _lib

    return wc.route(_lib.lib(), fmt, M, N, K)


def exact_problem(fmt, M, N, K, per_tensor, seed):
    """Inputs whose sums are exact in fp32 in any order: integer x, |x| <= 8; int8 codes |q| <= 127 (K 8 127 <= 2^22 for K <= 4096) with
    any positive fp32 scales (the chain applies them after the sum); e4m3 integer codes |q| <= 15 with power-of-two scales that differ
    per row.  The bias is any bf16."""
    assert K <= 4096
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randint(-8, 9, (M, K), generator=g).to(torch.bfloat16)
    ns = 1 if per_tensor else N
    if fmt == "int8":
        q = torch.randint(-127, 128, (N, K), generator=g).to(torch.int8)
        s = (torch.rand(ns, generator=g) * 0.02 + 1e-3).to(torch.float32)
    else:
        q = torch.randint(-15, 16, (N, K), generator=g).to(torch.float32).to(torch.float8_e4m3fn)
        s = torch.exp2((torch.arange(ns) * 5 % 13 - 8).to(torch.float32))
    bias = (torch.randn(N, generator=g) * 3).to(torch.bfloat16)
    d = _dev()
    return x.to(d), q.to(d), s.to(d), bias.to(d)


def run_exact(fmt, M, N, K, with_bias, per_tensor, seed, offset=False):
    x, q, s, bias = exact_problem(fmt, M, N, K, per_tensor, seed)
    ref = R.linear(R.FMTS[fmt], x, q, s, bias if with_bias else None)
    if offset:  # scale at a 4-byte, bias at a 2-byte offset from a 16-byte boundary
        s = torch.cat([s.new_zeros(1), s])[1:]
        bias = torch.cat([bias.new_zeros(1), bias])[1:]
        assert s.data_ptr() % 16 == 4 and bias.data_ptr() % 16 == 2
    buf = Guarded(M, N, torch.bfloat16, _dev())
    _op(fmt)(x, q, s, bias if with_bias else None, out=buf.out)
    torch.cuda.synchronize()
    check(buf, ref_bits=R.bits(ref), route=_lib_route(fmt, M, N, K))


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("idx", range(len(wc.CASES)), ids=["%s-%dx%dx%d" % c for c in wc.CASES])
def test_exact_every_route_case(idx, with_bias):
    fmt, M, N, K = wc.CASES[idx]
    run_exact(fmt, M, N, K, with_bias, per_tensor=idx % 3 == 0, seed=idx)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", [(129, 1040, 528), (257, 1000, 144), (33, 1040, 2064), (16, 1000, 4096)],
                         ids=["tile-129x1040x528", "tile-257x1000x144", "stream-33x1040x2064", "stream-16x1000x4096"])
@pytest.mark.parametrize("fmt", FMT_NAMES)
def test_exact_many_column_tiles(fmt, shape, with_bias):
    """The derivation picks the cheapest shape per requirement, so its wide cases have few k steps: here many column tiles (17 of the
    tiled form, the last one ragged, three row tiles) WITH several k steps and a partial last one, both forms."""
    M, N, K = shape
    assert _lib_route(fmt, M, N, K)["kernel"] == ("tile" if M > 64 else "stream")
    run_exact(fmt, M, N, K, with_bias, per_tensor=False, seed=200 + M)


def _first_per_kernel():
    from ao_amd import _lib

    seen, out = set(), []
    for c in wc.CASES:
        key = (c[0], wc.signature(_lib.lib(), c)[1])
        if key not in seen and c[2] > 16 and c[1] > 1:
            seen.add(key)
            out.append(c)
    return out


def test_exact_with_scale_and_bias_at_small_offsets():
    cases = _first_per_kernel()
    assert len(cases) == 4
    for i, (fmt, M, N, K) in enumerate(cases):
        run_exact(fmt, M, N, K, True, per_tensor=False, seed=100 + i, offset=True)


@pytest.mark.parametrize("fmt", FMT_NAMES)
@pytest.mark.parametrize("gran", ["row", "tensor"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
def test_golden_outputs_bit_for_bit(fmt, gran, with_bias):
    x, bias = _gbf("x"), _gbf("bias")
    q, s = _gcodes(fmt, f"{fmt}_{gran}_q"), torch.from_numpy(GOLDEN[f"{fmt}_{gran}_s"]).to(_dev())
    want = _gbf(f"{fmt}_{gran}_y" if with_bias else f"{fmt}_{gran}_y_nobias")
    buf = Guarded(x.shape[0], q.shape[0], torch.bfloat16, _dev())
    _op(fmt)(x, q, s, bias if with_bias else None, out=buf.out)
    check(buf, ref_bits=R.bits(want))


def test_golden_one_hot_is_dequantize():
    q, s = _gcodes("e4m3", "onehot_q"), torch.from_numpy(GOLDEN["onehot_s"]).to(_dev())
    x = torch.eye(16, q.shape[1], dtype=torch.bfloat16, device=_dev())
    buf = Guarded(16, q.shape[0], torch.bfloat16, _dev())
    _op("e4m3")(x, q, s, out=buf.out)
    check(buf, ref_bits=R.bits(_gbf("onehot_y")))
    assert torch.equal(R.bits(buf.out), R.bits(_gbf("onehot_dequant")[:, :16].t()))


@pytest.mark.parametrize("form", [1, 2], ids=["stream", "tile"])
@pytest.mark.parametrize("fmt", FMT_NAMES)
def test_one_hot_rows_return_the_weight(fmt, form):
    """80 one-hot rows (two grid rows of the forced stream form, two row tiles of the tiled form) over K = 272: the first k, the last k,
    a mid-tile k and a spread of the others.  float8 returns dequantize()'s bits -- the per-element rounding of the weight; int8
    bf16(bf16(q) bf16(s))."""
    from ao_amd import ops
    from ao_amd.quantization import Float8Tensor, Int8Tensor

    torch.manual_seed(11)
    N, K, M = 40, 272, 80
    w = (torch.randn(N, K, device=_dev()) * torch.rand(N, 1, device=_dev()) * 3).to(torch.bfloat16)
    t = (Int8Tensor if fmt == "int8" else Float8Tensor).from_hp(w)
    ks = torch.tensor([0, K - 1, 77] + [(r * 37 + 5) % K for r in range(3, M)], device=_dev())
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=_dev())
    x[torch.arange(M, device=_dev()), ks] = 1
    if fmt == "int8":
        want = (t.qdata.to(torch.bfloat16).float() * t.scale.to(torch.bfloat16).float()).to(torch.bfloat16)[:, ks].t()
    else:
        want = t.dequantize()[:, ks].t()
        assert torch.equal(want, (t.qdata.float() * t.scale).to(torch.bfloat16)[:, ks].t())
    buf = Guarded(M, N, torch.bfloat16, _dev())
    ops.wo8_set_form(form)
    try:
        assert ops.wo8_route(R.FMTS[fmt], M, N, K)["kernel"] == ("wo8_stream_kernel", "wo8_tile_kernel")[form - 1]
        _op(fmt)(x, t.qdata, t.scale, out=buf.out)
    finally:
        ops.wo8_set_form(0)
    check(buf, ref_bits=R.bits(want.contiguous()))
    assert torch.equal(R.bits(R.linear(R.FMTS[fmt], x, t.qdata, t.scale)), R.bits(want.contiguous()))


def interval_problems(y, fmt, x, q, s, bias, K):
    """y against the float64 sum m64: every element inside [chain(m64 - d), chain(m64 + d)], d = 2 K 2^-24 S (the accumulation
    allowance of _parity.bound; the chain is monotone: its scale is positive), and the fraction equal to chain(m64)."""
    f = R.FMTS[fmt]
    m64, S = R.sums(f, x, q, s)
    d = 2.0 * K * 2.0 ** -24 * S
    lo, hi, mid = (R.chain(f, v, s, bias).double() for v in (m64 - d, m64 + d, m64))
    yd = y.double()
    inside = (yd >= lo) & (yd <= hi)
    eq = (yd == mid).double().mean().item()
    print("%s %s: inside %.6f, equal %.6f" % (fmt, tuple(y.shape), inside.double().mean().item(), eq))
    msgs = []
    if not bool(inside.all()):
        i, j = (int(v) for v in torch.nonzero(~inside)[0])
        msgs.append("%d elements outside the interval, first at (%d, %d): %r not in [%r, %r]"
                    % (int((~inside).sum()), i, j, yd[i, j].item(), lo[i, j].item(), hi[i, j].item()))
    return msgs, eq


@pytest.mark.parametrize("form", [1, 2], ids=["stream", "tile"])
@pytest.mark.parametrize("shape", [(17, 1000, 4096), (33, 272, 1040)], ids=["17x1000x4096", "33x272x1040"])
@pytest.mark.parametrize("fmt", FMT_NAMES)
def test_gaussian_inside_the_float64_interval(fmt, shape, form):
    from ao_amd import ops
    from ao_amd.quantization import Float8Tensor, Int8Tensor

    M, N, K = shape
    g = torch.Generator(device="cpu").manual_seed(M + N)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(_dev())
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(_dev())
    bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16).to(_dev())
    t = (Int8Tensor if fmt == "int8" else Float8Tensor).from_hp(w)
    buf = Guarded(M, N, torch.bfloat16, _dev())
    ops.wo8_set_form(form)
    try:
        _op(fmt)(x, t.qdata, t.scale, bias, out=buf.out)
    finally:
        ops.wo8_set_form(0)
    msgs, eq = interval_problems(buf.out, fmt, x, t.qdata, t.scale, bias, K)
    msgs = buf.guard_problems() + msgs
    if bool((buf.bits() == buf.sentinel).any()):
        msgs.append("elements left unwritten")
    assert not msgs, "; ".join(msgs)
    assert eq >= _parity.EQUAL_FRACTION, f"only {eq:.4f} of the elements equal chain(m64)"


# ---- the tensor subclasses ----------------------------------------------------------------------------------------------------------
def _configs():
    from ao_amd.quantization import Float8WeightOnlyConfig, Int8WeightOnlyConfig, PerRow, PerTensor

    return [("int8", Int8WeightOnlyConfig, PerRow()), ("int8", Int8WeightOnlyConfig, PerTensor()),
            ("e4m3", Float8WeightOnlyConfig, PerRow()), ("e4m3", Float8WeightOnlyConfig, PerTensor())]


def _exact_weight(n, k, gen):
    """bf16 [n, k] whose 8-bit casts are exact and whose sums with integer activations are exact in fp32: integers |i| <= 7 times a
    power of two per row, every row holding a 7.  e4m3: amax / 448 = 2^(e - 6) per row (per tensor: of the largest row), so the codes
    are i 2^(6 + e - emax), at most three significant bits, and dequantize() returns the weight itself.  int8: any weight is exact
    (K 8 127 <= 2^22)."""
    w = torch.randint(-7, 8, (n, k), generator=gen).to(torch.float32)
    w[:, 0] = 7
    return (w * torch.exp2((torch.arange(n) % 5 - 6).to(torch.float32)).reshape(n, 1)).to(torch.bfloat16)


def _quantized_linear(cfg_cls, gran, seed=3, exact=False):
    from ao_amd.quantization import quantize_

    torch.manual_seed(seed)
    lin = torch.nn.Linear(256, 48, bias=True).to(torch.bfloat16).to(_dev())
    if exact:
        with torch.no_grad():
            lin.weight.copy_(_exact_weight(48, 256, torch.Generator().manual_seed(seed)).to(_dev()))
    quantize_(lin, cfg_cls(granularity=gran))
    return lin


def _assert_matches_ref(y, fmt, x2, q, s, bias):
    """Bit for bit against wo8_ref: the callers' inputs have sums that are exact in fp32 (integer activations, _exact_weight)."""
    want = R.linear(R.FMTS[fmt], x2, q, s, bias)
    got = y.reshape(-1, y.shape[-1])
    bad = R.bits(got) != R.bits(want)
    assert not bool(bad.any()), "%d elements differ from wo8_ref, first at %r" % (int(bad.sum()), tuple(int(v) for v in torch.nonzero(bad)[0]))


@pytest.mark.parametrize("idx", range(4), ids=["int8-row", "int8-tensor", "e4m3-row", "e4m3-tensor"])
def test_quantize_and_linear(idx):
    from ao_amd.quantization import Float8Tensor, Int8Tensor, PerTensor

    fmt, cfg_cls, gran = _configs()[idx]
    lin = _quantized_linear(cfg_cls, gran, exact=True)
    w = lin.weight
    assert isinstance(w, Int8Tensor if fmt == "int8" else Float8Tensor) and isinstance(w, torch.nn.Parameter) and not w.requires_grad
    assert w.act_quant_kwargs is None
    assert tuple(w.scale.shape) == ((1, 1) if isinstance(gran, PerTensor) else (48, 1))
    assert type(w).__name__ in repr(lin)
    torch.manual_seed(4)
    x = torch.randint(-8, 9, (2, 3, 256), device=_dev()).to(torch.bfloat16)
    with torch.no_grad():
        y = lin(x)
        y2 = F.linear(x, w)
        y0 = lin(x[:0].reshape(0, 256))
        y00 = lin(x[:, :0])
    assert y.shape == (2, 3, 48) and y.dtype == torch.bfloat16
    assert y0.shape == (0, 48) and y00.shape == (2, 0, 48) and y0.dtype == torch.bfloat16
    x2 = x.reshape(-1, 256)
    _assert_matches_ref(y, fmt, x2, w.qdata, w.scale, lin.bias)
    _assert_matches_ref(y2, fmt, x2, w.qdata, w.scale, None)
    # a K shard keeps the scales of the full rows
    ws = w[:, :128]
    assert tuple(ws.scale.shape) == tuple(w.scale.shape) and ws.act_quant_kwargs is None
    with torch.no_grad():
        ys = F.linear(x[..., :128].contiguous(), ws)
    _assert_matches_ref(ys, fmt, x2[:, :128].contiguous(), w.qdata[:, :128].contiguous(), w.scale, None)
    # act_pre_scale is applied first
    if fmt == "e4m3":  # the exact weight went through the cast unchanged
        assert torch.equal(R.bits(w.dequantize()), R.bits(_exact_weight(48, 256, torch.Generator().manual_seed(3)).to(_dev())))
    pre = torch.exp2((torch.arange(256, device=_dev()) % 3 - 1).float()).to(torch.bfloat16)  # powers of two: x pre stays exact
    wp = type(w)(w.qdata, w.scale, w.block_size, w.dtype_, act_pre_scale=pre)
    with torch.no_grad():
        yp = F.linear(x, wp)
    _assert_matches_ref(yp, fmt, (x * pre).reshape(-1, 256), w.qdata, w.scale, None)
    if fmt == "e4m3":
        with torch.no_grad():
            ym = torch.mm(x2, w.t())
        assert torch.equal(R.bits(ym), R.bits(y2.reshape(-1, 48)))


@pytest.mark.parametrize("idx", [0, 2], ids=["int8", "e4m3"])
def test_compiled_equals_eager(idx):
    fmt, cfg_cls, gran = _configs()[idx]
    lin = _quantized_linear(cfg_cls, gran, seed=6)
    x = torch.randn(5, 256, dtype=torch.bfloat16, device=_dev())
    with torch.no_grad():
        eager = lin(x)
        compiled = torch.compile(lin, backend="aot_eager")(x)
    assert torch.equal(R.bits(eager), R.bits(compiled))


def test_refusals_name_their_reason():
    from ao_amd.quantization import Float8Tensor, Int8Tensor, MappingType

    torch.manual_seed(8)
    w = torch.randn(32, 64, device=_dev()).to(torch.bfloat16)
    x = torch.randn(4, 64, device=_dev()).to(torch.bfloat16)
    for cls in (Int8Tensor, Float8Tensor):
        t = cls.from_hp(w)
        for dt in (torch.float16, torch.float32):
            with pytest.raises(NotImplementedError, match="takes bfloat16 activations"):
                F.linear(x.to(dt), t)
        t3 = cls.from_hp(torch.stack([w, w]))
        with pytest.raises(AssertionError, match="select an expert"):
            F.linear(x, t3)
        assert F.linear(x, t3[1]).shape == (4, 32)
    with pytest.raises(NotImplementedError, match="symmetric weights"):
        F.linear(x, Int8Tensor.from_hp(w, mapping_type=MappingType.ASYMMETRIC))
    t3 = Float8Tensor.from_hp(torch.stack([w, w]))
    offs = torch.tensor([2, 4], dtype=torch.int32, device=_dev())
    with pytest.raises(NotImplementedError, match="weight-only Float8Tensor _grouped_mm"):
        torch._grouped_mm(x, t3.transpose(-2, -1), offs=offs)
