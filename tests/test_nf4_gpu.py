"""NF4 (QLoRA) weights on the GPU: the casts against the reference's recorded bytes and against the restated contracts, every code,
dequantize, every route case of the fused linear with exact-sum inputs bit for bit, one-hot rows, Gaussian inputs inside the float64
interval, the route's two paths, autograd, quantize_, graph capture and torch.compile (tests/nf4_ref.py, tests/nf4_cases.py,
tests/golden/nf4.npz)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _parity  # noqa: E402
import nf4_cases as nc  # noqa: E402
import nf4_ref as R  # noqa: E402
from _parity import Guarded, check  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nf4.npz"))
CASES = ["b64", "two", "straddle", "sb8a", "sb8b", "b32", "b128", "planted", "m0", "exact"]
LINEAR_CASES = [c for c in CASES if c != "planted"]


def _dev():
    return torch.device("cuda", 0)


def meta(c):
    return tuple(int(v) for v in GOLDEN[f"{c}_meta"])


def to_bf(bits_np, shape=None):
    """uint16 bf16 bits (numpy) -> a bf16 tensor on the GPU"""
    t = torch.from_numpy(np.ascontiguousarray(bits_np).view(np.int16).copy()).view(torch.bfloat16)
    return (t if shape is None else t.reshape(shape)).to(_dev())


def to_bits(t):
    """a bf16 tensor -> uint16 bits (numpy, flat)"""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(_dev())


def same(a, b):
    """equal bits, or a NaN in both (its sign and payload are the processor's)"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    isnan = lambda v: (v & 0x7FFF) > 0x7F80  # noqa: E731
    return a.shape == b.shape and bool(np.all((a == b) | (isnan(a) & isnan(b))))


class forced_stream:
    def __enter__(self):
        from ao_amd import ops

        ops.nf4_set_form(1)

    def __exit__(self, *exc):
        from ao_amd import ops

        ops.nf4_set_form(0)
        return False


def _lib_route(M, N, K, B, SB):
    from ao_amd import _lib

    return nc.route(_lib.lib(), M, N, K, B, SB)


# ---- 1. the casts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES)
def test_cast_equals_the_reference_bytes(c):
    """nf4_block_absmax + nf4_quantize under the RECORDED mean: every field the reference recorded."""
    from ao_amd import ops

    rows, cols, B, SB = meta(c)
    x = to_bf(GOLDEN[f"{c}_x"], (rows, cols))
    absmax = ops.nf4_block_absmax(x, B)
    assert np.array_equal(to_bits(absmax), GOLDEN[f"{c}_absmax"])
    codes, q, qf = ops.nf4_quantize(x, absmax, to_bf(GOLDEN[f"{c}_mean"]), B, SB)
    assert (codes.dtype, q.dtype, qf.dtype) == (torch.uint8, torch.int8, torch.bfloat16)
    assert np.array_equal(codes.cpu().numpy(), GOLDEN[f"{c}_codes"]), "codes differ from the reference's"
    assert same(to_bits(qf), GOLDEN[f"{c}_factors"]), "quantization factors differ from the reference's"
    keep = ~np.repeat(GOLDEN[f"{c}_m0"], SB)  # (m = 0: the reference's NaN -> int8 is undefined; the kernel writes 0)
    assert np.array_equal(q.cpu().numpy()[keep], GOLDEN[f"{c}_scalers"][keep]), "int8 scalers differ from the reference's"
    assert not q.cpu().numpy()[~keep].any()


@pytest.mark.parametrize("SB", [1, 2, 8, 256])
@pytest.mark.parametrize("B", [32, 64, 128])
def test_cast_equals_the_restatement_on_ragged_sizes(B, SB):
    """One scaler block (one BLOCK at SB = 1), one scaler block plus one, five: sizes ragged against the 256-lane workgroups of both
    kernels and the four scaler blocks a workgroup takes.  The mean is torch's; the restatement takes its bits."""
    from ao_amd import ops

    for nsb in (1, 2, 5):
        numel = B * SB * nsb
        g = torch.Generator().manual_seed(B + SB + nsb)
        x = (torch.randn(numel, generator=g) * torch.exp(torch.randn(numel // B, 1, generator=g)).expand(-1, B).reshape(-1)).to(torch.bfloat16)
        absmax = ops.nf4_block_absmax(x.to(_dev()), B)
        mean = absmax.mean()
        codes, q, qf = ops.nf4_quantize(x.to(_dev()), absmax, mean, B, SB)
        torch.cuda.synchronize()
        r_absmax, r_codes, r_q, r_qf, m0 = R.quantize(to_bits(x), B, SB, to_bits(mean))
        keep = ~np.repeat(m0, SB)
        assert np.array_equal(to_bits(absmax), r_absmax) and np.array_equal(codes.cpu().numpy(), r_codes), (B, SB, nsb)
        assert same(to_bits(qf), r_qf) and np.array_equal(q.cpu().numpy()[keep], r_q[keep]), (B, SB, nsb)


def test_to_nf4_end_to_end_on_the_exact_mean_case():
    """Every partial sum of this case's mean is exact in fp32, so torch's mean on the device is the recorded one in any order."""
    from ao_amd.quantization import to_nf4

    rows, cols, B, SB = meta("exact")
    t = to_nf4(to_bf(GOLDEN["exact_x"], (rows, cols)), B, SB)
    assert tuple(t.shape) == (rows, cols) and t.dtype == torch.bfloat16 and (t.block_size, t.scaler_block_size, t.n_blocks) == (B, SB, rows * cols // B)
    assert np.array_equal(to_bits(t.scaler_mean.reshape(1)), GOLDEN["exact_mean"])
    assert np.array_equal(t.quantized_data.cpu().numpy(), GOLDEN["exact_codes"])
    assert np.array_equal(t.quantized_scalers.cpu().numpy(), GOLDEN["exact_scalers"])
    assert np.array_equal(to_bits(t.quantization_factor), GOLDEN["exact_factors"])
    assert np.array_equal(to_bits(t.get_original_weight()), GOLDEN["exact_w"].reshape(-1))
    assert np.array_equal(to_bits(t.nf4), R.bf16.to_bits(R.TABLE_BF16))


def test_codes_exhaustive():
    """Blocks whose maximum is 1.0 hold every bf16 with |v| <= 1, +-0 and the subnormals included: v = x / 1 = x, and the code is the host
    table's (the reference's quantize_tensor_nearest over every pattern, tests/golden/nf4.npz)."""
    from ao_amd import ops

    pats = np.concatenate([np.arange(0, 0x3F81), np.arange(0x8000, 0xBF81)]).astype(np.uint16)
    per = 63
    nblk = -(-len(pats) // per)
    x = np.zeros((nblk, 64), dtype=np.uint16)
    x[:, 0] = 0x3F80
    flat = np.zeros(nblk * per, dtype=np.uint16)
    flat[:len(pats)] = pats
    x[:, 1:] = flat.reshape(nblk, per)
    xt = to_bf(x.reshape(-1))
    absmax = ops.nf4_block_absmax(xt, 64)
    assert bool((absmax == 1.0).all())
    codes, _, _ = ops.nf4_quantize(xt, absmax, absmax.mean(), 64, 1)
    assert np.array_equal(R.unpack(codes.cpu().numpy()), GOLDEN["code_table"][x.reshape(-1)])


# ---- 2. dequantize ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES)
def test_dequantize_equals_the_reference_bits(c):
    from ao_amd import ops

    rows, cols, B, SB = meta(c)
    w = ops.nf4_dequantize(dev(GOLDEN[f"{c}_codes"]), dev(GOLDEN[f"{c}_scalers"]), to_bf(GOLDEN[f"{c}_factors"]), to_bf(GOLDEN[f"{c}_mean"]), B, SB)
    assert w.dtype == torch.bfloat16 and tuple(w.shape) == (rows * cols,)
    assert same(to_bits(w), GOLDEN[f"{c}_w"])


def random_fields(numel, B, SB, seed):
    """hand-made fields: any codes, any int8 scalers (-128 and 127 among them), finite non-zero factors, any mean"""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (numel // 2,), generator=g).to(torch.uint8)
    q = torch.randint(-128, 128, (numel // B,), generator=g).to(torch.int8)
    q[0], q[-1] = -128, 127
    mag = torch.exp(torch.rand(numel // (B * SB), generator=g) * 6 - 0.7)                       # 0.5 .. 200
    qf = (mag * torch.where(torch.rand(mag.shape, generator=g) < 0.3, -1.0, 1.0)).to(torch.bfloat16)
    mean = (torch.randn((), generator=g) * 0.3).to(torch.bfloat16)
    return codes, q, qf, mean


@pytest.mark.parametrize("fmt", [(32, 1, 7), (64, 8, 33), (128, 2, 9), (64, 256, 3)], ids=lambda f: "B%d-SB%d-x%d" % f)
def test_dequantize_equals_the_restatement_on_random_fields(fmt):
    from ao_amd import ops

    B, SB, nsb = fmt
    numel = B * SB * nsb
    codes, q, qf, mean = random_fields(numel, B, SB, numel)
    assert set(R.unpack(codes.numpy()).tolist()) == set(range(16)) and int(q.min()) == -128 and int(q.max()) == 127
    assert bool(torch.isfinite(qf.float()).all()) and bool((qf != 0).all())
    w = ops.nf4_dequantize(codes.to(_dev()), q.to(_dev()), qf.to(_dev()), mean.to(_dev()), B, SB)
    assert np.array_equal(to_bits(w), R.dequantize(codes.numpy(), q.numpy(), to_bits(qf), to_bits(mean.reshape(1)), B, SB))


# ---- 3. exact sums, every route case, the stream form forced --------------------------------------------------------------------------------
def assert_exact(S, unit, what):
    """Every term is a multiple of `unit` (asserted by the caller on the operands) and the absolute terms of an output sum to at most
    2^24 units: every partial sum, in any order, is an integer below 2^24 units -- exact in fp32."""
    assert float(S.max()) <= 2.0 ** 24 * unit, "%s: sum of |terms| %.6g exceeds 2^24 units of %g" % (what, float(S.max()), unit)


def exact_problem(M, N, K, B, SB, seed):
    """mean = 0, factor 64, int8 scalers in {16, 32, 64}: block scalers 1/4, 1/2, 1; any codes; integer x, {-1, 0, 1} from K = 2048 up:
    terms are multiples of 2^-13 (table: 2^-11) and sum to at most 2048 in absolute value per output."""
    g = torch.Generator().manual_seed(seed)
    numel = N * K
    codes = torch.randint(0, 256, (numel // 2,), generator=g).to(torch.uint8)
    q = torch.tensor([16, 32, 64], dtype=torch.int8)[torch.randint(0, 3, (numel // B,), generator=g)]
    qf = torch.full((numel // (B * SB),), 64.0, dtype=torch.bfloat16)
    mean = torch.zeros((), dtype=torch.bfloat16)
    xmax = max(1, min(8, 2048 // K))
    x = torch.randint(-xmax, xmax + 1, (M, K), generator=g).to(torch.bfloat16)
    w = R.weight(codes.numpy(), q.numpy(), to_bits(qf), to_bits(mean.reshape(1)), B, SB, (N, K))
    unit = 2.0 ** -13
    assert torch.equal(x.double(), x.double().round()) and torch.equal(w.double() / unit, (w.double() / unit).round())
    assert_exact(x.double().abs() @ w.double().abs().t(), unit, "nf4")
    return x, codes, q, qf, mean, w


@pytest.mark.parametrize("idx", range(len(nc.CASES)), ids=["%dx%dx%d-B%d-SB%d" % c for c in nc.CASES])
def test_exact_every_route_case(idx):
    from ao_amd import ops

    M, N, K, B, SB = nc.CASES[idx]
    x, codes, q, qf, mean, w = exact_problem(M, N, K, B, SB, idx)
    buf = Guarded(M, N, torch.bfloat16, _dev())
    d = _dev()
    with forced_stream():
        route = _lib_route(M, N, K, B, SB)
        assert route["kernel"] == "stream"
        ops.nf4_linear(x.to(d), codes.to(d), q.to(d), qf.to(d), mean.to(d), N, K, B, SB, out=buf.out)
    torch.cuda.synchronize()
    check(buf, ref_bits=R.bits(R.linear(x, w)).to(d), route=route)


# ---- 4. one-hot rows -------------------------------------------------------------------------------------------------------------------------
def test_one_hot_rows_return_dequantize():
    """80 one-hot rows (two grid rows of the forced stream form) over K = 320 at (64, 2): five blocks a row, so scaler blocks end inside
    rows, and scalers that differ from block to block: the first k, the last k, a mid-block k and a spread of the others return
    dequantize's bits.  (A -0.0 weight returns +0.0: the accumulator starts at +0.0.)"""
    from ao_amd import ops
    from ao_amd.quantization import to_nf4

    torch.manual_seed(11)
    N, K, M, B, SB = 40, 320, 80, 64, 2
    w = (torch.randn(N, K, device=_dev()) * torch.exp(torch.randn(N, K // B, 1, device=_dev())).expand(-1, -1, B).reshape(N, K)).to(torch.bfloat16)
    t = to_nf4(w, B, SB)
    deq = t.get_original_weight()
    assert len(set(R.unpack(t.quantized_data.cpu().numpy()).tolist())) == 16
    assert len(set(t.quantized_scalers.cpu().tolist())) > 40 and len(set(to_bits(t.quantization_factor).tolist())) > 40
    assert np.array_equal(to_bits(deq), R.dequantize(t.quantized_data.cpu().numpy(), t.quantized_scalers.cpu().numpy(),
                                                     to_bits(t.quantization_factor), to_bits(t.scaler_mean.reshape(1)), B, SB))
    ks = torch.tensor([0, K - 1, 77] + [(r * 37 + 5) % K for r in range(3, M)], device=_dev())
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=_dev())
    x[torch.arange(M, device=_dev()), ks] = 1
    want = (deq[:, ks].t() + 0.0).contiguous()
    buf = Guarded(M, N, torch.bfloat16, _dev())
    with forced_stream():
        r = ops.nf4_linear_route(M, N, K, B, SB)
        assert r["kernel"] == "nf4_stream_kernel" and r["grid"][1] == 2
        ops.nf4_linear(x, t.quantized_data, t.quantized_scalers, t.quantization_factor, t.scaler_mean, N, K, B, SB, out=buf.out)
    check(buf, ref_bits=R.bits(want))


# ---- 5. Gaussian inputs ------------------------------------------------------------------------------------------------------------------------
def interval_problems(y, m64, S, K, chain):
    """y against the float64 sum m64: every element inside [chain(m64 - d), chain(m64 + d)], d = 2 K 2^-24 S (the accumulation allowance
    of _parity.bound; the chain is monotone), and the fraction equal to chain(m64)."""
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


@pytest.mark.parametrize("shape", [(17, 1000, 4096, 256), (33, 17, 512, 8)], ids=["17x1000x4096-SB256", "33x17x512-SB8"])
def test_gaussian_inside_the_float64_interval(shape):
    """The forced stream form: every element inside the interval, and at least _parity.EQUAL_FRACTION of them equal to bf16(float64 sum)
    (measured on an MI355X: inside 1.0 and 1.0, equal 0.99982 and 0.99822)."""
    from ao_amd import ops
    from ao_amd.quantization import to_nf4

    M, N, K, SB = shape
    g = torch.Generator(device="cpu").manual_seed(M + N)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(_dev())
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(_dev())
    t = to_nf4(w, 64, SB)
    buf = Guarded(M, N, torch.bfloat16, _dev())
    with forced_stream():
        assert ops.nf4_linear_route(M, N, K, 64, SB)["kernel"] == "nf4_stream_kernel"
        ops.nf4_linear(x, t.quantized_data, t.quantized_scalers, t.quantization_factor, t.scaler_mean, N, K, 64, SB, out=buf.out)
    m64, S = R.sums(x, t.get_original_weight())
    msgs, eq = interval_problems(buf.out.cpu(), m64, S, K, R.chain)
    msgs = buf.guard_problems() + msgs
    if bool((buf.bits() == buf.sentinel).any()):
        msgs.append("elements left unwritten")
    assert not msgs, "; ".join(msgs)
    assert eq >= _parity.EQUAL_FRACTION, f"only {eq:.4f} of the elements equal bf16(float64 sum)"


# ---- 6. the route's two paths ----------------------------------------------------------------------------------------------------------------
def test_not_fused_routes_are_dequantize_then_linear():
    """Above the seam, and where blocks straddle rows, ops.nf4_linear IS F.linear(x, nf4_dequantize(...)): the same bits."""
    from ao_amd import ops
    from ao_amd.quantization import to_nf4

    g = torch.Generator().manual_seed(21)
    for (M, N, K), why in (((300, 128, 256), "above the seam"), ((5, 512, 96), "K % block_size != 0")):
        w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16).to(_dev())
        x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(_dev())
        t = to_nf4(w)
        assert ops.nf4_linear_route(M, N, K)["kernel"] == "not fused", why
        fields = (t.quantized_data, t.quantized_scalers, t.quantization_factor, t.scaler_mean)
        y = ops.nf4_linear(x, *fields, N, K)
        want = F.linear(x, ops.nf4_dequantize(*fields).view(N, K))
        assert torch.equal(R.bits(y), R.bits(want)), why
        assert torch.equal(R.bits(F.linear(x, t)), R.bits(want)) and torch.equal(R.bits(x @ t.t()), R.bits(want)), why


# ---- 7. autograd ---------------------------------------------------------------------------------------------------------------------------------
def test_linear_nf4_forward_is_fused_and_backward_is_dequantize():
    from ao_amd import ops
    from ao_amd.quantization import linear_nf4, to_nf4

    g = torch.Generator().manual_seed(31)
    M, N, K = 5, 96, 256
    w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16).to(_dev())
    t = to_nf4(w, 64, 8)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(_dev()).requires_grad_(True)
    go = torch.randn(M, N, generator=g).to(torch.bfloat16).to(_dev())
    assert ops.nf4_linear_route(M, N, K, 64, 8)["kernel"] == "nf4_stream_kernel"
    y = linear_nf4(x, t)
    y.backward(go)
    deq = t.get_original_weight()
    assert torch.equal(R.bits(x.grad), R.bits(go @ deq)) and t.grad is None and not t.requires_grad
    m64, S = R.sums(x.detach(), deq)
    assert bool(((y.detach().cpu().double() - m64).abs() <= _parity.bound(m64, S, K, torch.bfloat16)).all())
    # a 3-D activation and a bias through F.linear
    x3 = torch.randn(2, 3, K, generator=g).to(torch.bfloat16).to(_dev())
    bias = torch.randn(N, generator=g).to(torch.bfloat16).to(_dev())
    y3 = F.linear(x3, t, bias)
    assert tuple(y3.shape) == (2, 3, N) and torch.equal(R.bits(y3), R.bits(linear_nf4(x3.reshape(6, K), t).reshape(2, 3, N) + bias))


@pytest.mark.parametrize("c", LINEAR_CASES)
def test_recorded_forward_and_grad_input_are_met(c):
    """The recorded forward and grad_input are the reference's CPU sums: met inside _parity.bound."""
    from ao_amd.quantization import NF4Tensor, linear_nf4
    from ao_amd.quantization.nf4_tensor import NF4_TABLE, SubclassTensorArgs

    rows, cols, B, SB = meta(c)
    m = SubclassTensorArgs(torch.Size((rows, cols)), (cols, 1), 0, torch.bfloat16, _dev(), False)
    t = NF4Tensor(m, B, rows * cols // B, SB, dev(GOLDEN[f"{c}_scalers"]), to_bf(GOLDEN[f"{c}_factors"]), to_bf(GOLDEN[f"{c}_mean"]).reshape(()),
                  dev(GOLDEN[f"{c}_codes"]), torch.tensor(NF4_TABLE, dtype=torch.bfloat16, device=_dev()))
    x = to_bf(GOLDEN[f"{c}_in"], (5, cols)).requires_grad_(True)
    go = to_bf(GOLDEN[f"{c}_go"], (5, rows))
    y = linear_nf4(x, t)
    y.backward(go)
    w = to_bf(GOLDEN[f"{c}_w"], (rows, cols))
    for got, want, (m64, S), K in ((y.detach(), to_bf(GOLDEN[f"{c}_y"], (5, rows)), R.sums(x.detach(), w), cols),
                                   (x.grad, to_bf(GOLDEN[f"{c}_gi"], (5, cols)), R.sums(go, w.t().contiguous()), rows)):
        b = _parity.bound(m64, S, K, torch.bfloat16)
        assert bool(((got.cpu().double() - m64).abs() <= b).all()) and bool(((want.cpu().double() - m64).abs() <= b).all())


# ---- 8. quantize_ and the subclass ----------------------------------------------------------------------------------------------------------
def _mlp(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(256, 128, bias=True), torch.nn.ReLU(), torch.nn.Linear(128, 128, bias=False)).to(torch.bfloat16).to(_dev())


def test_quantize_and_the_subclass_surface():
    from ao_amd.prototype.nf4_api import NF4WeightOnlyConfig
    from ao_amd.quantization import NF4Tensor, linear_nf4, quantize_, to_nf4

    model, plain = _mlp(3), _mlp(3)
    quantize_(model, NF4WeightOnlyConfig())
    x = torch.randn(7, 256, dtype=torch.bfloat16, device=_dev())
    w0, w2 = to_nf4(plain[0].weight.detach()), to_nf4(plain[2].weight.detach())
    for p, w in ((model[0].weight, w0), (model[2].weight, w2)):
        assert isinstance(p, NF4Tensor) and isinstance(p, torch.nn.Parameter) and not p.requires_grad
        assert (p.block_size, p.scaler_block_size) == (64, 256) and tuple(p.shape) == tuple(w.shape)
        for name in ("quantized_data", "quantized_scalers", "quantization_factor", "scaler_mean", "nf4"):
            assert torch.equal(getattr(p, name), getattr(w, name)), name
    with torch.no_grad():
        y = model(x)
        want = linear_nf4(torch.relu(linear_nf4(x, w0) + plain[0].bias), w2)
    assert torch.equal(R.bits(y), R.bits(want))
    t = w0
    deq = t.get_original_weight()
    assert torch.equal(R.bits(t.to(torch.bfloat16)), R.bits(deq)) and t.to(torch.float32).dtype == torch.float32
    assert torch.equal(t.to(torch.float32), deq.float())
    c = t.cpu()
    assert isinstance(c, NF4Tensor) and c.device.type == "cpu" and c.quantized_data.device.type == "cpu"
    back = c.cuda()
    assert isinstance(back, NF4Tensor) and back.device.type == "cuda" and torch.equal(R.bits(back.get_original_weight()), R.bits(deq))
    assert torch.equal(R.bits(c.to(_dev()).get_original_weight()), R.bits(deq))
    for u in (t.clone(), t.detach()):
        assert isinstance(u, NF4Tensor) and torch.equal(R.bits(u.get_original_weight()), R.bits(deq))
    tt = t.t()
    assert tuple(tt.shape) == (256, 128) and torch.equal(R.bits(tt.to(torch.bfloat16)), R.bits(deq.t()))
    assert torch.equal(R.bits(x @ tt), R.bits(linear_nf4(x, t)))
    with pytest.raises(NotImplementedError, match="aten.view"):
        t.view(-1)


# ---- 9. capture and torch.compile -------------------------------------------------------------------------------------------------------------
def test_cast_dequantize_and_linear_replay_from_a_graph():
    """No host read anywhere: absmax, torch's mean, the cast that reads it through its pointer, dequantize and the fused linear replay on
    new data with the eager bits."""
    from ao_amd import ops

    g = torch.Generator().manual_seed(5)
    N, K, B, SB = 64, 256, 64, 8
    w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16).to(_dev())
    x = torch.randn(4, K, generator=g).to(torch.bfloat16).to(_dev())

    def run(wt, xt):
        a = ops.nf4_block_absmax(wt, B)
        mean = a.mean()
        codes, q, qf = ops.nf4_quantize(wt, a, mean, B, SB)
        return codes, q, qf, mean, ops.nf4_dequantize(codes, q, qf, mean, B, SB), ops.nf4_linear(xt, codes, q, qf, mean, N, K, B, SB)

    assert ops.nf4_linear_route(4, N, K, B, SB)["kernel"] == "nf4_stream_kernel"
    sw, sx = w.clone(), x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(sw, sx)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(sw, sx)
    w2, x2 = (w * 1.5 + 0.01).to(torch.bfloat16), (x * 3 + 1).to(torch.bfloat16)
    sw.copy_(w2)
    sx.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, run(w2, x2)):
        assert torch.equal(got.reshape(-1).view(torch.uint8), want.reshape(-1).view(torch.uint8))


def test_compiled_op_equals_eager():
    """The dispatcher op on plain tensors under torch.compile (compiling a module that holds the subclass is out of scope)."""
    import ao_amd.torch_ops  # noqa: F401
    from ao_amd.quantization import to_nf4

    g = torch.Generator().manual_seed(6)
    N, K = 64, 256
    t = to_nf4((torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16).to(_dev()), 64, 8)
    x = torch.randn(5, K, generator=g).to(torch.bfloat16).to(_dev())

    def f(x, codes, q, qf, mean):
        return torch.ops.ao_mi355.nf4_linear(x * 2, codes, q, qf, mean, N, K, 64, 8) + 1

    args = (x, t.quantized_data, t.quantized_scalers, t.quantization_factor, t.scaler_mean)
    eager = f(*args)
    compiled = torch.compile(f, backend="aot_eager", fullgraph=True)(*args)
    assert torch.equal(R.bits(eager), R.bits(compiled))
