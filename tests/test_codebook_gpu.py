"""Codebook (k-means) weights on the GPU: the assignment and the Lloyd step against float64, the dequantize and the fused linear bit for
bit, and the tensor end to end.  Bounds are those of the fp32 arithmetic, never measured numbers."""
import pytest
import torch
import torch.nn.functional as F

import _parity
from ao_amd import _lib, ops
from ao_amd.prototype import CodebookQuantizedTensor, CodebookWeightOnlyConfig
from ao_amd.quantization import quantize_

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
FORMATS = [(d, k) for d in (1, 2, 4, 8) for k in (16, 256)]
N_RAGGED = 2 * 2048 + 5  # past a second workgroup for every d (a workgroup's tile is 1024 or 2048 rows), ragged last tile
N_STRIDE = 1025 * 1024 + 5  # more tiles of 1024 rows than a launch has workgroups (1024): a workgroup walks a second tile


def _seam(d):
    return 48 if d <= 2 else 64  # the route's seam by block width (codebook_kernels.hip: cb_stream_max_rows)


def _gauss(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _assert_optimal(x, table, codes):
    """S_code >= max_j S_j - 2 eps, eps = (d + 2) 2^-24 max_j(sum_i |x_i c_ji| + |c_j|^2 / 2): the fp32 dot product's error bound."""
    x, t, codes = x.double().cpu(), table.double().cpu(), codes.cpu().long().flatten()
    half = 0.5 * (t * t).sum(1)
    S = x @ t.T - half
    mag = (x.abs() @ t.abs().T + half)
    mag = torch.where(torch.isnan(mag), torch.zeros_like(mag), mag).max(1).values
    eps = (x.shape[1] + 2) * U * mag
    best = torch.where(torch.isnan(S), torch.full_like(S, -torch.inf), S).max(1).values
    got = S[torch.arange(len(x)), codes]
    assert bool((got >= best - 2 * eps).all()), f"{int((~(got >= best - 2 * eps)).sum())} rows off the float64 optimum"


def _int_table(d, k):
    """k distinct rows of small integers: the digits of j in the smallest base that holds k in d digits"""
    base = 2
    while base ** d < k:
        base += 1
    j = torch.arange(k)
    return torch.stack([(j // base ** i) % base for i in range(d)], 1).float() - (base // 2)


def _pack_u4(codes):
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).to(torch.uint8)


def _fields(d, k, n, kk, sb, seed=0, ints=False):
    g = torch.Generator().manual_seed(seed)
    full = torch.randint(0, k, (n, kk // d), generator=g, dtype=torch.uint8)
    if ints:
        table = torch.randint(-8, 9, (k, 1, d), generator=g).to(torch.bfloat16)
        scales = (2.0 ** torch.randint(-2, 3, (n, kk // sb, 1), generator=g)).to(torch.bfloat16)
    else:
        table = torch.randn(k, 1, d, generator=g).to(torch.bfloat16)
        scales = (torch.rand(n, kk // sb, 1, generator=g) + 0.5).to(torch.bfloat16)
    w64 = table.double().view(k, d)[full.long()].view(n, kk) * scales.double().expand(n, kk // sb, sb).reshape(n, kk)
    codes = _pack_u4(full) if k == 16 else full
    return codes.to(DEV), table.to(DEV), scales.to(DEV), w64, full


@pytest.mark.parametrize("n", [1, 323, N_RAGGED])
@pytest.mark.parametrize("d,k", FORMATS)
def test_assignment_is_optimal_in_float64(d, k, n):
    x, table = _gauss(n, d, seed=n), _gauss(k, d, seed=k + d)
    _assert_optimal(x, table, ops.codebook_assign(x.to(DEV), table.to(DEV)))


@pytest.mark.parametrize("d,k", [(1, 16), (2, 16), (4, 256), (8, 256)])
def test_assignment_exact_cases(d, k):
    table = _int_table(d, k)
    idx = torch.randint(0, k, (N_RAGGED,), generator=torch.Generator().manual_seed(1))
    assert torch.equal(ops.codebook_assign(table[idx].to(DEV), table.to(DEV)).cpu().long(), idx)
    dup = table.clone()
    dup[7] = dup[3]  # equal scores: the lower index
    assert torch.equal(ops.codebook_assign(dup[idx].to(DEV), dup.to(DEV)).cpu().long(), torch.where(idx == 7, torch.full_like(idx, 3), idx))
    nan = table.clone()
    nan[5] = float("nan")
    codes = ops.codebook_assign(table[idx].to(DEV), nan.to(DEV)).cpu().long()
    assert not bool((codes == 5).any()) and torch.equal(codes[idx != 5], idx[idx != 5])
    assert int(ops.codebook_assign(table[:3].to(DEV), torch.full_like(table, float("nan")).to(DEV)).sum()) == 0  # every score NaN: code 0


@pytest.mark.parametrize("d,k", FORMATS)
def test_lloyd_step_means_counts_and_empty_entries(d, k):
    x, table = _gauss(N_RAGGED, d, seed=3), _gauss(k, d, seed=4)
    table[k - 2] = 1000.0  # far from every row: no member
    new, counts, codes = ops.codebook_lloyd_step(x.to(DEV), table.to(DEV), return_codes=True)
    new, counts, codes = new.cpu(), counts.cpu().long(), codes.cpu().long()
    _assert_optimal(x, table, codes)
    assert int(counts.sum()) == N_RAGGED and torch.equal(counts, torch.bincount(codes, minlength=k))
    assert counts[k - 2] == 0 and torch.equal(new[counts == 0].view(torch.int32), table[counts == 0].view(torch.int32))
    x64 = x.double()
    sums = torch.zeros(k, d, dtype=torch.float64).index_add_(0, codes, x64)
    mags = torch.zeros(k, d, dtype=torch.float64).index_add_(0, codes, x64.abs())
    cnt = counts.clamp(min=1).double()[:, None]
    bound = ((cnt - 1) * U * mags + U * sums.abs()) / cnt
    live = counts > 0
    assert bool(((new.double() - sums / cnt).abs() <= bound)[live].all())


def test_lloyd_step_where_a_workgroup_walks_two_tiles():
    """The sums of a second tile land in the same LDS partial; the plain assignment walks the same grid and gives the same codes."""
    d, k = 4, 16
    x, table = _gauss(N_STRIDE, d, seed=7), _gauss(k, d, seed=8)
    new, counts, codes = ops.codebook_lloyd_step(x.to(DEV), table.to(DEV), return_codes=True)
    assert torch.equal(ops.codebook_assign(x.to(DEV), table.to(DEV)), codes)
    new, counts, codes = new.cpu(), counts.cpu().long(), codes.cpu().long()
    _assert_optimal(x, table, codes)
    assert torch.equal(counts, torch.bincount(codes, minlength=k)) and int(counts.min()) > 0
    x64 = x.double()
    sums = torch.zeros(k, d, dtype=torch.float64).index_add_(0, codes, x64)
    mags = torch.zeros(k, d, dtype=torch.float64).index_add_(0, codes, x64.abs())
    cnt = counts.double()[:, None]
    assert bool(((new.double() - sums / cnt).abs() <= ((cnt - 1) * U * mags + U * sums.abs()) / cnt).all())


# K of two scale blocks and of one; sb = 12 and 6: the element-wise path (scale blocks off the 8 grid), where the format has it (d | sb);
# K = 12: 36 elements, a last piece of 4
DEQUANT_CASES = [(d, k, kk, sb) for d, k in FORMATS for kk, sb in ((64, 32), (64, 64), (24, 12), (12, 6)) if sb % d == 0]


@pytest.mark.parametrize("d,k,kk,sb", DEQUANT_CASES)
def test_dequantize_is_the_float64_product_rounded_once(d, k, kk, sb):
    n = 3
    codes, table, scales, w64, full = _fields(d, k, n, kk, sb, seed=d + k)
    if k == 16:
        assert torch.equal(ops.codebook_pack_u4(full.to(DEV)), codes)
    out = torch.full((n * kk + 8,), -7.0, dtype=torch.bfloat16, device=DEV)
    _lib.check(_lib.lib().ao_codebook_dequantize(codes.data_ptr(), table.data_ptr(), scales.data_ptr(), out.data_ptr(), n, kk, d, k, sb, None))
    torch.cuda.synchronize()
    assert torch.equal(out[:n * kk].cpu().view(torch.int16), w64.to(torch.bfloat16).flatten().view(torch.int16))
    assert bool((out[n * kk:] == -7.0).all())
    assert torch.equal(ops.codebook_dequantize(codes, table, scales), out[:n * kk].view(n, kk))


# (K, N, sb): the smallest K; K of 13 runs (a partial last step), ragged N; K of 10 steps over 8 waves (uneven), sb = K; one tile, sb < K
LINEAR_SHAPES = [(32, 16, 32), (416, 40, 32), (1184, 40, 1184), (1184, 16, 32)]


@pytest.mark.parametrize("m", [1, 5, 16, 17, 48, 49, 64, 65])  # at and above either seam
@pytest.mark.parametrize("d,k", FORMATS)
def test_linear_exact_sums_on_every_route(d, k, m):
    for kk, n, sb in LINEAR_SHAPES:
        codes, table, scales, w64, _ = _fields(d, k, n, kk, sb, seed=kk + m, ints=True)
        x = torch.randint(-4, 5, (m, kk), generator=torch.Generator().manual_seed(m)).to(torch.bfloat16)
        ref = (x.double() @ w64.T).to(torch.bfloat16).view(torch.int16)  # sums of small integers: exact in fp32 in any order
        assert ops.codebook_linear_kernel_name(m, n, kk, d, k, sb) == ("codebook_stream_kernel" if m <= _seam(d) else "not fused")
        for form in (0, 1):
            ops.codebook_linear_set_form(form)
            try:
                y = ops.codebook_linear(x.to(DEV), codes, table, scales)
            finally:
                ops.codebook_linear_set_form(0)
            assert torch.equal(y.cpu().view(torch.int16), ref), (kk, n, sb, form)


@pytest.mark.parametrize("d,k", FORMATS)
def test_linear_one_hot_rows_return_the_dequantized_rows(d, k):
    codes, table, scales, _, _ = _fields(d, k, 40, 64, 32, seed=9)
    y = ops.codebook_linear(torch.eye(64, dtype=torch.bfloat16, device=DEV), codes, table, scales)
    assert torch.equal(y.view(torch.int16), ops.codebook_dequantize(codes, table, scales).T.contiguous().view(torch.int16))


@pytest.mark.parametrize("d,k,m,n,kk,sb", [(8, 256, 7, 72, 1024, 256), (1, 16, 33, 40, 2048, 2048)])
def test_linear_gaussian_inside_the_fp32_bound(d, k, m, n, kk, sb):
    codes, table, scales, w64, _ = _fields(d, k, n, kk, sb, seed=5)
    w64 = w64.to(torch.bfloat16).double()  # the bit-exact dequantized weight
    x = _gauss(m, kk, seed=6).to(torch.bfloat16)
    y = ops.codebook_linear(x.to(DEV), codes, table, scales)
    m64, S = x.double() @ w64.T, x.double().abs() @ w64.abs().T
    assert bool(((y.cpu().double() - m64).abs() <= _parity.bound(m64, S, kk, torch.bfloat16)).all())


def _sqnr(w, q):
    w, q = w.float(), q.float()
    return float(20 * torch.log10(torch.linalg.vector_norm(w) / torch.linalg.vector_norm(w - q)))


@pytest.mark.parametrize("dtype,k", [(torch.uint4, 16), (torch.uint8, 256)])
def test_from_float_recovers_a_weight_of_k_distinct_values(dtype, k):
    values = (torch.arange(k, dtype=torch.float32) - k + 1) / 256  # k distinct bf16 values, the largest 0: below the 1.0 every block holds
    w = values[torch.arange(24 * 128) % (k - 1)].view(24, 128).clone()  # every value but the last, fewer than 2^16 times: exact sums
    w[:, 1::64] = 1.0  # the k-th value, the maximum of every scale block of 64: scales of exactly 1.0
    w = w.to(torch.bfloat16).to(DEV)
    assert len(torch.unique(w)) == k
    q = CodebookQuantizedTensor.from_float(w, (1, 1), dtype, 64)
    assert torch.equal(q.dequantize().view(torch.int16), w.view(torch.int16))


# the reference's own test tensor (test_codebook_quant.py) and its bar of 30 dB; the others: the reference's CPU value minus 1 dB
@pytest.mark.parametrize("dtype,block,sb,floor", [(torch.uint8, (1, 1), 64, 30.0), (torch.uint4, (1, 1), 256, 18.90), (torch.uint8, (1, 4), 256, 9.28),
                                                   (torch.uint8, (1, 8), 256, 3.73), (torch.uint4, (1, 2), 64, 8.29)])
def test_from_float_sqnr_on_the_reference_tensor(dtype, block, sb, floor):
    torch.manual_seed(123)
    w = torch.randn(100, 256, dtype=torch.float32).to(torch.bfloat16).to(DEV)
    s = _sqnr(w, CodebookQuantizedTensor.from_float(w, block, dtype, sb).dequantize())
    print(f"SQNR {dtype} {block} sb={sb}: {s:.2f} dB")
    assert s >= floor


def test_quantize_model_codes_are_optimal_and_linear_matches_dequantize(monkeypatch):
    from ao_amd.prototype import codebook as cb

    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(128, 96, bias=False, dtype=torch.bfloat16), torch.nn.Linear(96, 32, bias=False, dtype=torch.bfloat16)).to(DEV)
    w0 = model[0].weight.detach().clone()
    tables, fit = [], cb._fit_kmeans  # the UNROUNDED tables, as from_float's k-means returns them
    monkeypatch.setattr(cb, "_fit_kmeans", lambda *a, **kw: tables.append(fit(*a, **kw)) or tables[-1])
    quantize_(model, CodebookWeightOnlyConfig(dtype=torch.uint8, block_size=(1, 4), scale_block_size=32))
    q = model[0].weight
    assert type(q) is CodebookQuantizedTensor and type(model[1].weight) is CodebookQuantizedTensor
    _assert_optimal(cb._scales_and_data(w0, 4, 32)[1], tables[0], q.codes)
    x = torch.randn(5, 128, device=DEV).to(torch.bfloat16)
    for layer in model:  # each layer against float64 on its own input and its bit-exact dequantized weight
        y, w64, x64 = layer(x), layer.weight.dequantize().double().cpu(), x.double().cpu()
        m64, S = x64 @ w64.T, x64.abs() @ w64.abs().T
        assert bool(((y.double().cpu() - m64).abs() <= _parity.bound(m64, S, x.shape[1], torch.bfloat16)).all())
        x = y


def test_assign_dequantize_and_linear_replay_from_a_graph():
    d, k, n, kk, sb, m = 8, 256, 40, 256, 64, 4
    codes, table, scales, _, _ = _fields(d, k, n, kk, sb, seed=11)
    x = _gauss(m, kk, seed=12).to(torch.bfloat16).to(DEV)
    rows, tab32 = _gauss(N_RAGGED, d, seed=13).to(DEV), _gauss(k, d, seed=14).to(DEV)
    eager = (ops.codebook_assign(rows, tab32), ops.codebook_dequantize(codes, table, scales), ops.codebook_linear(x, codes, table, scales))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.codebook_linear(x, codes, table, scales)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = (ops.codebook_assign(rows, tab32), ops.codebook_dequantize(codes, table, scales), ops.codebook_linear(x, codes, table, scales))
    for _ in range(3):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)
