"""Int8 mixed-precision training on the GPU, bit for bit against a few lines of torch-CPU / numpy: the casts in both directions, the GEMM in
every layout at the edges of its 128 x 128 tile and of its three 64-deep LDS stages, the autograd Function under three configs and both
quantize_ routes, and one graph capture.  Integer sums are exact and the epilogue is three fp32 operations, so nothing here has a tolerance.

The issue's cast case "an entry that lands on +-127.5 before rounding" cannot exist: scale = bf16(amax / 127) is off by at most 2^-9, so
|x| / scale peaks at 127.33 (amax 1.484375).  The inputs hold that row, and exact ties (2.5, -3.5 under scale 1) where they can exist."""
import copy
import functools

import numpy as np
import pytest
import torch

from ao_amd import ops
from ao_amd.prototype import quantized_training as Q
from ao_amd.quantization import quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def bits(t):
    return t.cpu().contiguous().view(torch.int16)


def ref_cast(t, eps=1e-12):
    scale = t.abs().amax(1) / 127
    inv = 1.0 / scale.float().clip(eps)
    v = t.float() * inv.view(-1, 1)
    return v.round().clip(-128, 127).to(torch.int8), scale


def ref_mm(a, b, sa, sb):
    """a int8 [M, Kc], b int8 [N, Kc] -> bf16 [M, N]: the int64 product, then np.float32 multiplies in the kernel's order."""
    acc = a.numpy().astype(np.int64) @ b.numpy().astype(np.int64).T
    y = acc.astype(np.float32) * sa.float().numpy()[:, None] * sb.float().numpy()[None, :]
    return torch.from_numpy(y).to(BF16)


def cast_input(R, C):
    g = torch.Generator().manual_seed(R * 1000 + C)
    x = (torch.randn(R, C, generator=g) * torch.exp2(torch.randint(-20, 7, (R, C), generator=g).float())).clamp(-100, 100).to(BF16)
    x[:, 3] = 0  # a zero column
    x[-1, 5] = -0.0
    x[-1, :3] = torch.tensor([127.0, 2.5, -3.5], dtype=BF16)  # amax 127, scale 1: the ties go to even, 2 and -4
    if R > 2:
        x[0] = 0
        x[0, 1], x[0, 2] = -1.484375, 1.4765625  # the largest overshoot a bf16 amax reaches: v = -127.33
        x[1] = 0  # a zero row
        x[2, 0] = 2.5  # column 0 has amax 127 too: a tie down the column
    return x


# beyond the issue's shapes, the sizes at which the casts take another path: 2, 4 and no held pieces a thread, more than one 4096-column chunk
@pytest.mark.parametrize("R,C", [(r, c) for r in (1, 17, 130) for c in (16, 80, 272)] + [(4, 4112), (4, 8208), (4, 16400)])
def test_cast_bytes(R, C):
    x = cast_input(R, C)
    want_rq, want_rs = ref_cast(x)
    want_cq, want_cs = ref_cast(x.T)
    assert want_rq[-1, 1] == 2 and want_rq[-1, 2] == -4 and not want_cq[3].any() and want_cs[3] == 0
    assert R < 3 or (want_rq[0, 1] == -127 and not want_rq[1].any() and want_rs[1] == 0 and want_cq[0, 2] == 2)
    xg = x.to(DEV)
    rows, cols, both = ops.int8_train_quantize(xg), ops.int8_train_quantize(xg, rows=False, cols=True), ops.int8_train_quantize(xg, cols=True)
    for got_r, got_c in ((rows, cols), (both[:2], both[2:])):
        assert torch.equal(got_r[0].cpu(), want_rq) and torch.equal(bits(got_r[1]), bits(want_rs))
        assert torch.equal(got_c[0].cpu(), want_cq.T) and torch.equal(bits(got_c[1]), bits(want_cs))
    q, s = Q.quantize_int8_rowwise(xg.T)  # a transposed view is the column cast
    assert torch.equal(q.cpu(), want_cq) and torch.equal(bits(s), bits(want_cs))


def test_stochastic_rounding():
    x = cast_input(17, 272)
    q, s = ops.int8_train_quantize(x.to(DEV), sr_seed=7, sr_offset=3)
    v = x.float() * (1.0 / s.cpu().float().clip(1e-12)).view(-1, 1)
    lo, q = v.floor(), q.cpu().float()
    assert torch.equal(bits(s), bits(ref_cast(x)[1]))
    assert ((q == lo.clip(-128, 127)) | (q == (lo + 1).clip(-128, 127))).all() and (q != lo).any()
    assert torch.equal(q[v == lo], v[v == lo]) and (v == lo).sum() > 272  # exact integers do not move
    assert torch.equal(ops.int8_train_quantize(x.to(DEV), sr_seed=7, sr_offset=3)[0].cpu().float(), q)
    assert not torch.equal(ops.int8_train_quantize(x.to(DEV), sr_seed=8, sr_offset=3)[0].cpu().float(), q)
    assert not torch.equal(ops.int8_train_quantize(x.to(DEV), cols=True, sr_seed=7, sr_offset=4)[0].cpu().float(), q)
    assert torch.equal(ops.int8_train_quantize(x.to(DEV), cols=True, sr_seed=7, sr_offset=3)[0].cpu().float(), q)  # the two-pass form, same stream
    # unbiased: 2^16 elements at k + 0.25 exactly (k in -32 .. 31 keeps them bf16 values) in a row of amax 127, scale 1
    k = (torch.arange(2 ** 16) % 64 - 32).float()
    row = torch.cat([k + 0.25, torch.full((16,), 127.0)]).to(BF16).view(1, -1)
    assert torch.equal(row[0, : 2 ** 16].float(), k + 0.25)
    got = Q.quantize_int8_rowwise(row.to(DEV), stochastic_rounding=True)[0].cpu().float()[0, : 2 ** 16]
    up = (got == k + 1).float().mean().item()
    assert ((got == k) | (got == k + 1)).all() and abs(up - 0.25) <= 0.0102, up  # six standard deviations of Binomial(2^16, 1/4)


@functools.lru_cache(maxsize=None)
def mm_case(M, N, Kc, hot=False):
    rng = np.random.default_rng(M * 7919 + N * 31 + Kc)
    a = torch.from_numpy(rng.integers(126, 128, size=(M, Kc), dtype=np.int8) if hot else rng.integers(-128, 128, size=(M, Kc), dtype=np.int8))
    b = torch.from_numpy(np.repeat(rng.choice(np.array([127, -128], dtype=np.int8), size=(N, 1)), Kc, axis=1) if hot else rng.integers(-128, 128, size=(N, Kc), dtype=np.int8))
    a[0, 0] = -128
    sa = torch.from_numpy((rng.random(M, dtype=np.float32) + 0.5) / 64).to(BF16)
    sb = torch.from_numpy((rng.random(N, dtype=np.float32) + 0.5) / 64).to(BF16)
    return a, b, sa, sb, ref_mm(a, b, sa, sb)


def run_mm(a, b, sa, sb, a_t, b_t):
    a = a.T.contiguous() if a_t else a
    b = b.T.contiguous() if b_t else b
    return ops.int8_train_mm(a.to(DEV), b.to(DEV), sa.to(DEV), sb.to(DEV), a_t=a_t, b_t=b_t)


# tile 128 x 128, 3 stages of 64: rows and columns at 1 or 16, T - 16, T + 16; the contraction below one step, one step, a step and a ragged
# tail, and the ring wrapped once (64 * 4 + 16); 1 where both operands have it outermost.  (An operand's contiguous dimension is a multiple of 16.)
MM_CASES = [(a_t, b_t, M, N, Kc) for a_t, b_t in ((False, False), (False, True), (True, True), (True, False))
            for M in ((16 if a_t else 1), 112, 144) for N in (16, 112, 144) for Kc in ((1,) if a_t and b_t else ()) + (16, 64, 80, 272)]


@pytest.mark.parametrize("a_t,b_t,M,N,Kc", MM_CASES)
def test_mm_bits(a_t, b_t, M, N, Kc):
    a, b, sa, sb, want = mm_case(M, N, Kc)
    got = run_mm(a, b, sa, sb, a_t, b_t)
    assert got.shape == (M, N) and torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("a_t,b_t", [(False, False), (False, True), (True, True)])
def test_mm_rounds_a_sum_above_2_to_24_once(a_t, b_t):
    a, b, sa, sb, want = mm_case(16, 16, 2064, hot=True)  # |acc| near 127 * 127 * 2064 = 2^24.99: the int32 -> fp32 conversion rounds
    acc = a.numpy().astype(np.int64) @ b.numpy().astype(np.int64).T
    assert (np.abs(acc) > 2 ** 24).any() and (acc.astype(np.float32).astype(np.int64) != acc).any()
    assert torch.equal(bits(run_mm(a, b, sa, sb, a_t, b_t)), bits(want))


def ref_dyn_mm(A, B):
    a_q, a_s = ref_cast(A)
    b_q, b_s = ref_cast(B.T)
    return ref_mm(a_q, b_q, a_s, b_s)


def sqnr(got, want):
    return 10 * torch.log10(want.float().pow(2).sum() / (got.float() - want.float()).pow(2).sum()).item()


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("flags", [(True, True, True), (True, False, False), (False, True, True)])
def test_function_and_quantize_routes(flags, bias):
    M, K, N = 48, 80, 48
    g = torch.Generator().manual_seed(11)
    x, w, go = torch.randn(M, K, generator=g).to(BF16), (torch.randn(N, K, generator=g) * 0.1).to(BF16), torch.randn(M, N, generator=g).to(BF16)
    b = torch.randn(N, generator=g).to(BF16) if bias else None
    xg, wg, gog, bg = x.to(DEV), w.to(DEV), go.to(DEV), (b.to(DEV) if bias else None)
    # the restated chain: the CPU cast composed with the int64 GEMM; a GEMM whose flag is False is torch.mm in bf16
    out = ref_dyn_mm(x, w.T).to(DEV) if flags[0] else xg @ wg.T
    out = out + bg if bias else out
    want = [out, ref_dyn_mm(go, w).to(DEV) if flags[1] else gog @ wg, ref_dyn_mm(x.T, go).T.to(DEV) if flags[2] else gog.T @ xg, gog.sum(0)]
    if all(flags):  # int8 against fp32 autograd: the CPU chain clears the bar first, then the GPU is asked to
        x32, w32 = x.float().requires_grad_(), w.float().requires_grad_()
        torch.nn.functional.linear(x32, w32, b.float() if bias else None).backward(go.float())
        exact = [torch.nn.functional.linear(x32, w32, b.float() if bias else None).detach(), x32.grad, w32.grad]
        assert min(sqnr(r.cpu(), e) for r, e in zip(want, exact)) > 30

    def run(module):
        xin = xg.clone().requires_grad_()
        y = module(xin)
        y.backward(gog)
        return [y.detach(), xin.grad, module.weight.grad, module.bias.grad if bias else gog.sum(0)]

    lin = torch.nn.Linear(K, N, bias=bias, dtype=BF16, device=DEV)
    with torch.no_grad():
        lin.weight.copy_(wg)
        if bias:
            lin.bias.copy_(bg)
    config = Q.Int8MixedPrecisionTrainingConfig(*flags)
    direct = copy.deepcopy(lin)
    direct.forward = lambda t: Q._Int8MixedPrecisionTrainingLinearFunction.apply(t, direct.weight, direct.bias, config)
    by_subclass, by_swap = copy.deepcopy(lin), copy.deepcopy(lin)
    quantize_(by_subclass, config)
    quantize_(by_swap, Q.Int8MixedPrecisionTrainingConfig(*flags, module_swap=True))
    assert isinstance(by_subclass.weight, Q.Int8MixedPrecisionTrainingLinearWeight) and isinstance(by_swap, Q.Int8MixedPrecisionTrainingLinear)
    assert torch.equal(by_subclass.weight.to_original(), wg) and type(by_subclass.weight.to_original()) is torch.Tensor
    for module in (direct, by_subclass, by_swap):
        results = run(module)
        for got, exp in zip(results, want):
            assert got.shape == exp.shape and torch.equal(bits(got), bits(exp))
        assert not all(flags) or min(sqnr(r.cpu(), e) for r, e in zip(results[:3], exact)) > 30
    if all(flags):
        assert torch.equal(bits(Q._dynamic_int8_mm(gog, wg)), bits(want[1])) and torch.equal(bits(Q._dynamic_int8_mm(xg, wg.T)), bits(ref_dyn_mm(x, w.T)))


def test_graph_replays_give_the_eager_bytes():
    torch.manual_seed(3)
    lin = torch.nn.Linear(80, 48, dtype=BF16, device=DEV)
    quantize_(lin, Q.Int8MixedPrecisionTrainingConfig())
    x = torch.randn(48, 80, device=DEV).to(BF16).requires_grad_()
    g = torch.randn(48, 48, device=DEV).to(BF16)

    def step():
        x.grad = lin.weight.grad = lin.bias.grad = None
        y = lin(x)
        y.backward(g)
        return y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.detach().clone() for t in (step(), x.grad, lin.weight.grad, lin.bias.grad)]
    torch.cuda.current_stream().wait_stream(side)
    x.grad = lin.weight.grad = lin.bias.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation on the path would fail the capture
        y = lin(x)
        y.backward(g)
    for _ in range(3):
        for t in (y, x.grad, lin.weight.grad, lin.bias.grad):
            t.detach().zero_()
        graph.replay()
        for got, exp in zip((y, x.grad, lin.weight.grad, lin.bias.grad), eager):
            assert torch.equal(bits(got), bits(exp))
