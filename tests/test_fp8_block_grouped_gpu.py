"""The blockwise float8 grouped GEMM on the GPU (token groups against MoE experts; 1 x 128 activation blocks, 128 x 128 weight blocks):
the fp32 chain bit for bit on exact sums and float64 on Gaussian operands on every case and with each form forced, reproducible
launches, the fixture recorded from the reference's emulation, the reference's own end-to-end bar, Float8BlockwiseExpertWeights,
torch.compile and the refusals (tests/fp8_block_grouped_ref.py, fixture tests/golden/fp8_block_grouped.npz).

K_FLOOR and EQUAL are the dense blockwise tests' constants for this instruction (tests/test_fp8_block_gpu.py): conditions, not targets.
Every Gaussian case prints its k_needed and equal fraction before it asserts."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_block_grouped_ref as G  # noqa: E402
import fp8_block_ref as R  # noqa: E402
from _parity import SENTINEL2, Guarded, check, k_needed, oracle_round  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "fp8_block_grouped.npz"))
with open(os.path.join(os.path.dirname(HERE), "include", "ao_mi355.h")) as fh:
    SEAM = int(re.search(r"#define AO_FP8_BLOCK_GROUPED_STREAM_MAX_ROWS (\d+)", fh.read()).group(1))  # on the mean group size
K_FLOOR = 896
EQUAL = 0.95
STREAM, TILE = "fp8_block_grouped_stream_kernel", "fp8_block_grouped_tile_kernel"
# (group sizes, N, K, unwritten tail rows)
CASES = [([1], 128, 128, 0), ([0, 1, 16, 17], 130, 256, 0), ([15, 0, 33], 257, 1152, 5), ([2, 0, 0, 5, 1, 0, 3, 1], 384, 2304, 0),
         ([64, 1, 0], 144, 1152, 3), ([0, 0, 40], 128, 384, 0), ([129, 0, 200], 130, 256, 0), ([256, 256], 256, 256, 0),
         ([129, 255, 116], 256, 256, 0)]
_SPARSE = [0] * 256
_SPARSE[0], _SPARSE[100], _SPARSE[255] = 3, 17, 1
CASES.append((_SPARSE, 128, 128, 0))  # E = 256, three non-empty groups
FORCED = [CASES[2], CASES[6]]
IDS = lambda c: f"E{len(c[0])}-M{sum(c[0])}+{c[3]}-N{c[1]}-K{c[2]}"  # noqa: E731
# The (m-tiles, waves) instances of the stream form that no case above launches, with the form forced: mean group sizes of 2 / 17 / 33
# rows take 1 / 2 / 4 m-tiles; one column tile (N = 16) asks for the most waves, the K / 128 k steps cap them.  (case, pair)
STREAM_PAIRS = [(([3, 1], 16, 512, 0), (1, 4)), (([3, 1], 16, 1024, 0), (1, 8)), (([20, 14], 16, 128, 0), (2, 1)),
                (([20, 14], 16, 256, 0), (2, 2)), (([20, 14], 16, 512, 0), (2, 4)), (([20, 14], 16, 2048, 0), (2, 16)),
                (([40, 26], 16, 128, 0), (4, 1)), (([40, 26], 16, 512, 0), (4, 4)), (([40, 26], 16, 1024, 0), (4, 8))]
EXACT_CASES = CASES + [case for case, _ in STREAM_PAIRS]  # what _exact and _exact_case index


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _np(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _want(sizes, tail):
    """The product route's kernel: it keys on ceil(M_total / E), the tail rows included (the host does not read offs)."""
    e = len(sizes)
    return STREAM if (sum(sizes) + tail + e - 1) // e <= SEAM else TILE


def _run(aq, a_s, wq, ws, offs, N, buf=None):
    """One launch on numpy codes and scales into a guarded buffer."""
    from ao_amd import ops

    buf = buf or Guarded(aq.shape[0], N, torch.bfloat16, _dev())
    ops.fp8_block_grouped_mm(_t(aq).view(torch.float8_e4m3fn), _t(a_s), _t(wq).view(torch.float8_e4m3fn), _t(ws), _t(offs), out=buf.out)
    torch.cuda.synchronize()
    return buf


class _forced:
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from ao_amd import ops

        ops.fp8_block_grouped_mm_set_form(self.form)

    def __exit__(self, *exc):
        from ao_amd import ops

        ops.fp8_block_grouped_mm_set_form(0)
        return False


# ---- exact sums ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact(i):
    """test_fp8_block_gpu._exact_operands' recipe per expert: integer e4m3 codes |q| <= 15, power-of-two scales that differ per (row, kb)
    and per (expert, nb, kb) within 2^7 of one another: every partial sum, in any order, is exact in fp32 (asserted), so the output bits
    are the chain's whatever the kernel's order.  The operands and the chain, computed once per case."""
    from oracle import fp8_ref

    sizes, N, K, tail = EXACT_CASES[i]
    E, M = len(sizes), sum(sizes) + tail
    g = np.random.default_rng(2000 + i)
    kb, nb = K // 128, (N + 127) // 128
    aq = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (M, K)).astype(np.float32))
    wq = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (E, N, K)).astype(np.float32))
    a_s = np.exp2(g.integers(-2, 2, (M, kb))).astype(np.float32)
    ws = np.exp2(g.integers(-2, 3, (E, nb, kb))).astype(np.float32)
    offs = G.offs_of(sizes)
    _, S = G.grouped_f64(aq, a_s, wq, ws, offs)
    assert S.max() / 2.0 ** -4 < 2.0 ** 24, "the sums of this case are not exact in fp32 in every order"
    assert a_s.max() * ws.max() / (a_s.min() * ws.min()) <= 2.0 ** 7
    ref = G.grouped_chain_bits(aq, a_s, wq, ws, offs)
    return aq, a_s, wq, ws, offs, ref


def _exact_case(i, want):
    from ao_amd import ops

    sizes, N, K, tail = EXACT_CASES[i]
    rows = sum(sizes)
    assert ops.fp8_block_grouped_mm_kernel_name(rows + tail, N, K, len(sizes)) == want
    aq, a_s, wq, ws, offs, ref = _exact(i)
    buf = _run(aq, a_s, wq, ws, offs, N)
    check(buf, ref_bits=_t(ref.view(np.int16)), written_rows=rows)
    assert len(np.unique(ref[:rows])) > min(rows * N, 64) // 2  # the outputs tell the elements apart


@pytest.mark.parametrize("i", range(len(CASES)), ids=[IDS(c) for c in CASES])
def test_exact_sums_pin_every_index(i):
    _exact_case(i, _want(CASES[i][0], CASES[i][3]))


@pytest.mark.parametrize("form,want", [(1, STREAM), (2, TILE)])
@pytest.mark.parametrize("case", FORCED, ids=[IDS(c) for c in FORCED])
def test_exact_sums_with_each_form_forced(form, want, case):
    from ao_amd import ops

    with _forced(form):
        _exact_case(CASES.index(case), want)
    sizes, N, K, tail = case
    assert ops.fp8_block_grouped_mm_kernel_name(sum(sizes) + tail, N, K, len(sizes)) == _want(sizes, tail)


@pytest.mark.parametrize("case,pair", STREAM_PAIRS, ids=[IDS(c) for c, _ in STREAM_PAIRS])
def test_exact_sums_on_the_remaining_stream_instances(case, pair):
    from ao_amd import ops

    sizes, N, K, tail = case
    with _forced(1):
        route = ops.fp8_block_grouped_mm_route(sum(sizes) + tail, N, K, len(sizes))
        assert (route["m_tiles"], route["waves"]) == pair
        _exact_case(EXACT_CASES.index(case), STREAM)


# ---- Gaussian operands against float64 -----------------------------------------------------------------------------------------------------
def _cast_experts(w):
    """Our 128 x 128 cast of bf16 [E, N, K] experts of any N: every expert's rows padded with zeros to a multiple of 128 (they join no
    amax), one cast over the [E Npad, K] view, the first N rows of every expert kept."""
    from ao_amd import ops

    E, N, K = w.shape
    pad = (-N) % 128
    wp = torch.cat([w, w.new_zeros(E, pad, K)], dim=1) if pad else w
    q, s = ops.fp8_quantize_block_128x128(wp.reshape(E * (N + pad), K))
    return q.reshape(E, N + pad, K)[:, :N].contiguous(), s.reshape(E, (N + pad) // 128, K // 128)


@functools.lru_cache(maxsize=None)
def _gaussian(i):
    """Operands through our own casts (the recipe of test_fp8_block_gpu._operands per expert) and the float64 reference, once per case."""
    from ao_amd import ops

    sizes, N, K, tail = CASES[i]
    E, M = len(sizes), sum(sizes) + tail
    g = torch.Generator().manual_seed(300 + i)
    x = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).to(torch.bfloat16)
    w = (torch.randn(E, N, K, generator=g) * 0.05).to(torch.bfloat16)
    aq, a_s = ops.fp8_quantize_block_1x128(x.to(_dev()))
    wq, ws = _cast_experts(w.to(_dev()))
    offs = G.offs_of(sizes)
    y64, S = G.grouped_f64(_np(aq), a_s.cpu().numpy(), _np(wq), ws.cpu().numpy(), offs)
    return _np(aq), a_s.cpu().numpy(), _np(wq), ws.cpu().numpy(), offs, y64, S


def _gaussian_case(i):
    from ao_amd import ops

    sizes, N, K, tail = CASES[i]
    rows = sum(sizes)
    aq, a_s, wq, ws, offs, y64, S = _gaussian(i)
    buf = _run(aq, a_s, wq, ws, offs, N)
    ref64, St = _t(y64), _t(S)
    eq = (buf.out[:rows] == oracle_round(ref64[:rows], torch.bfloat16)).double().mean().item()
    print(f"fp8_block_grouped {ops.fp8_block_grouped_mm_kernel_name(rows + tail, N, K, len(sizes))} {IDS(CASES[i])}: "
          f"k_needed {k_needed(buf.out[:rows], ref64[:rows], St[:rows], torch.bfloat16):.0f} equal {eq:.4f}")
    check(buf, ref64=ref64, S=St, K=K, k_floor=K_FLOOR, equal=EQUAL, written_rows=rows)
    return buf


@pytest.mark.parametrize("i", range(len(CASES)), ids=[IDS(c) for c in CASES])
def test_gaussian_against_float64(i):
    from ao_amd import ops

    sizes, N, K, tail = CASES[i]
    assert ops.fp8_block_grouped_mm_kernel_name(sum(sizes) + tail, N, K, len(sizes)) == _want(sizes, tail)
    _gaussian_case(i)


@pytest.mark.parametrize("form,want", [(1, STREAM), (2, TILE)])
@pytest.mark.parametrize("case", FORCED, ids=[IDS(c) for c in FORCED])
def test_gaussian_with_each_form_forced(form, want, case):
    from ao_amd import ops

    sizes, N, K, tail = case
    with _forced(form):
        assert ops.fp8_block_grouped_mm_kernel_name(sum(sizes) + tail, N, K, len(sizes)) == want
        _gaussian_case(CASES.index(case))


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("case", FORCED, ids=[IDS(c) for c in FORCED])
def test_a_second_launch_gives_the_same_bits(form, case):
    i = CASES.index(case)
    aq, a_s, wq, ws, offs, _, _ = _gaussian(i)
    with _forced(form):
        buf = _run(aq, a_s, wq, ws, offs, case[1])
        first = buf.bits().clone()
        buf.poison(SENTINEL2)  # another sentinel: what the second launch leaves alone shows
        _run(aq, a_s, wq, ws, offs, case[1], buf)
    rows = sum(case[0])
    assert not buf.guard_problems()
    assert torch.equal(buf.bits()[:rows], first[:rows])
    assert bool((buf.bits()[rows:] == buf.sentinel).all())


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "B"])
def test_fixture_within_the_bound_and_no_farther_than_the_emulation(case):
    aq, a_s, wq, ws, offs = (GOLDEN[f"{case}_{k}"] for k in ("aq", "as", "wq", "ws", "offs"))
    N, K, rows = wq.shape[1], wq.shape[2], int(offs[-1])
    y64, S = G.grouped_f64(aq, a_s, wq, ws, offs)
    buf = _run(aq, a_s, wq, ws, offs, N)
    ours, emulated = G.l2_to(y64, _bits(buf.out), rows), G.l2_to(y64, GOLDEN[f"{case}_emulated"], rows)
    print(f"fixture {case}: k_needed {k_needed(buf.out, _t(y64), _t(S), torch.bfloat16):.0f}; l2 to float64: ours {ours:.5g}, emulated {emulated:.5g}")
    check(buf, ref64=_t(y64), S=_t(S), K=K, k_floor=K_FLOOR, equal=EQUAL, written_rows=rows)
    assert ours <= emulated


# ---- end to end, at the reference's own bar ------------------------------------------------------------------------------------------------
def _compute_error_db(ref64, y):
    """torchao.quantization.utils.compute_error: 20 log10(|ref| / |ref - y|)."""
    return (20 * torch.log10(torch.linalg.norm(ref64) / torch.linalg.norm(ref64 - y.double()))).item()


def _grouped_product_f64(A, W, offs):
    """The float64 product of the bf16 inputs: A [M, K], W [E, N, K] on the CPU."""
    y = torch.zeros(A.shape[0], W.shape[1], dtype=torch.float64)
    for e, b, t in G.groups(offs, A.shape[0]):
        y[b:t] = A[b:t].double() @ W[e].double().t()
    return y


@pytest.mark.parametrize("offs", [[256, 512], [129, 384, 500]], ids=["256-512", "129-384-500"])
def test_end_to_end_reaches_the_reference_threshold(offs):
    """The recipe of test/prototype/moe_training/test_fp8_blockwise_grouped_mm.py:44-68, inputs drawn on the CPU: 27 dB is its threshold."""
    from ao_amd.prototype import fp8_blockwise_grouped_mm

    torch.manual_seed(0)
    E, M = len(offs), offs[-1]
    A = torch.randn(M, 256, dtype=torch.bfloat16)
    W = torch.randn(E, 256, 256, dtype=torch.bfloat16)
    o = torch.tensor(offs, dtype=torch.int32)
    out = fp8_blockwise_grouped_mm(A.to(_dev()), W.to(_dev()).transpose(-2, -1), o.to(_dev()))
    assert out.shape == (M, 256) and out.dtype == torch.bfloat16
    db = _compute_error_db(_grouped_product_f64(A, W, offs), out.cpu())
    print(f"end to end offs {offs}: {db:.2f} dB")
    assert db >= 27.0


# ---- Float8BlockwiseExpertWeights ----------------------------------------------------------------------------------------------------------
def _experts_and_tokens(E=3, N=256, K=384, M=23, seed=21):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(E, N, K, generator=g) * 0.05).to(torch.bfloat16).to(_dev())
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(_dev())
    offs = torch.tensor([5, 5, M - 3][:E], dtype=torch.int32, device=_dev())  # an empty group, three rows past offs[-1]
    return w, A, offs


def test_expert_weights_from_hp_is_the_cast_per_expert():
    from ao_amd import ops
    from ao_amd.prototype import Float8BlockwiseExpertWeights
    from ao_amd.quantization import Float8Tensor, PerBlock

    w, A, offs = _experts_and_tokens()
    ew = Float8BlockwiseExpertWeights.from_hp(w.transpose(-2, -1))
    assert ew.shape == torch.Size((3, 384, 256)) and ew.data.dtype == torch.float8_e4m3fn and tuple(ew.scale.shape) == (3, 2, 3)
    for e in range(3):
        q, s = ops.fp8_quantize_block_128x128(w[e])
        assert torch.equal(ew.data[e].view(torch.uint8), q.view(torch.uint8)) and torch.equal(ew.scale[e], s)
    rq, rs = G.cast_experts(_bits(w))
    assert R.same_codes(_np(ew.data), rq)
    np.testing.assert_array_equal(ew.scale.cpu().numpy(), rs)
    # from_float8_tensors equals stacking
    ts = [Float8Tensor.from_hp(w[e], granularity=PerBlock([128, 128])) for e in range(3)]
    st = Float8BlockwiseExpertWeights.from_float8_tensors(ts)
    assert torch.equal(st.data.view(torch.uint8), ew.data.view(torch.uint8)) and torch.equal(st.scale, ew.scale)
    with pytest.raises(ValueError, match="Float8BlockwiseExpertWeights.from_float8_tensors"):
        Float8BlockwiseExpertWeights.from_float8_tensors([Float8Tensor.from_hp(w[0])])


def test_prebuilt_experts_and_a_bf16_view_give_the_same_bits():
    from ao_amd import ops
    from ao_amd.prototype import Float8BlockwiseExpertWeights, fp8_blockwise_grouped_mm

    w, A, offs = _experts_and_tokens()
    ew = Float8BlockwiseExpertWeights.from_hp(w.transpose(-2, -1))
    y0 = fp8_blockwise_grouped_mm(A, ew, offs)
    y1 = fp8_blockwise_grouped_mm(A, w.transpose(-2, -1), offs)
    assert y0.dtype == torch.bfloat16 and tuple(y0.shape) == (23, 256)
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
    assert not bool(y0[20:].any()) and bool(y0[:20].any())  # rows past offs[-1] of a fresh output are zero
    # and both are the cast followed by the launch on codes, inside the float64 bound
    aq, a_s = ops.fp8_quantize_block_1x128(A)
    y2 = ops.fp8_block_grouped_mm(aq, a_s, ew.data, ew.scale, offs)
    assert torch.equal(y0.view(torch.int16), y2.view(torch.int16))
    y64, S = G.grouped_f64(_np(aq), a_s.cpu().numpy(), _np(ew.data), ew.scale.cpu().numpy(), offs.cpu().numpy())
    buf = Guarded(20, 256, torch.bfloat16, _dev())
    buf.out.copy_(y0[:20])
    check(buf, ref64=_t(y64[:20]), S=_t(S[:20]), K=384, k_floor=K_FLOOR, equal=EQUAL)


def test_raw_checkpoint_tensors_with_ragged_n_run():
    """weight / weight_scale_inv stacked as a loader does, N = 130: the first 130 rows of a cast at N = 256 with its scales."""
    from ao_amd.prototype import Float8BlockwiseExpertWeights, fp8_blockwise_grouped_mm

    w, A, offs = _experts_and_tokens()
    full = Float8BlockwiseExpertWeights.from_hp(w.transpose(-2, -1))
    ragged = Float8BlockwiseExpertWeights(full.data[:, :130].contiguous(), full.scale.clone())
    assert ragged.shape == torch.Size((3, 384, 130))
    y = fp8_blockwise_grouped_mm(A, ragged, offs)
    assert tuple(y.shape) == (23, 130)
    assert torch.equal(y.view(torch.int16), fp8_blockwise_grouped_mm(A, full, offs)[:, :130].contiguous().view(torch.int16))


def test_torch_compile_fullgraph_bitwise():
    from ao_amd.prototype import Float8BlockwiseExpertWeights, fp8_blockwise_grouped_mm

    w, A, offs = _experts_and_tokens()
    ew = Float8BlockwiseExpertWeights.from_hp(w.transpose(-2, -1))

    def f(a, o):
        return fp8_blockwise_grouped_mm(a, ew, o)

    eager = f(A, offs)
    compiled = torch.compile(f, fullgraph=True)(A, offs)
    assert torch.equal(eager.view(torch.int16), compiled.view(torch.int16))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_op():
    from ao_amd import ops
    from ao_amd.prototype import Float8BlockwiseExpertWeights, fp8_blockwise_grouped_mm

    d = _dev()
    f8 = lambda *s: torch.zeros(*s, dtype=torch.float8_e4m3fn, device=d)  # noqa: E731
    ones = lambda *s: torch.ones(*s, device=d)  # noqa: E731
    offs = torch.tensor([2, 4], dtype=torch.int32, device=d)
    ok = (f8(4, 256), ones(4, 2), f8(2, 130, 256), ones(2, 2, 2), offs)
    assert tuple(ops.fp8_block_grouped_mm(*ok).shape) == (4, 130)
    bad = {
        "K % 128": (f8(4, 192), ones(4, 1), f8(2, 130, 192), ones(2, 2, 1), offs),
        "offs dtype": ok[:4] + (offs.to(torch.int64),),
        "offs length": ok[:4] + (torch.tensor([1, 2, 4], dtype=torch.int32, device=d),),
        "2-D weight codes": (ok[0], ok[1], f8(130, 256), ones(2, 2), offs),
        "a_scale shape": (ok[0], ones(4, 1), ok[2], ok[3], offs),
        "w_scale shape": (ok[0], ok[1], ok[2], ones(2, 1, 2), offs),
        "w_scale 2-D": (ok[0], ok[1], ok[2], ones(2, 2), offs),
    }
    for what, args in bad.items():
        with pytest.raises(RuntimeError, match="fp8_block_grouped_mm: "):
            ops.fp8_block_grouped_mm(*args)
            pytest.fail(what)
    ew = Float8BlockwiseExpertWeights(ok[2], ok[3])
    A = torch.zeros(4, 256, dtype=torch.bfloat16, device=d)
    for call in (lambda: fp8_blockwise_grouped_mm(A.float(), ew, offs), lambda: fp8_blockwise_grouped_mm(A.half(), ew, offs),
                 lambda: fp8_blockwise_grouped_mm(A, ew, offs.long()), lambda: fp8_blockwise_grouped_mm(A, ew, offs[:1]),
                 lambda: fp8_blockwise_grouped_mm(A[:, :128], ew, offs), lambda: fp8_blockwise_grouped_mm(A, ew, offs, out_dtype=torch.float32),
                 lambda: fp8_blockwise_grouped_mm(A, torch.zeros(2, 256, 130, device=d), offs)):
        with pytest.raises(ValueError, match="fp8_blockwise_grouped_mm: "):
            call()
