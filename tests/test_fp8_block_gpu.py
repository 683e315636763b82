"""Blockwise float8 linears on the GPU (1 x 128 activation blocks, 128 x 128 weight blocks): both casts against the reference's bytes, the
GEMM against the fp32 chain on exact sums and against float64 on Gaussian operands on every route, the fused cast against cast + GEMM,
the operand lane map, quantize_, raw checkpoint tensors and torch.compile (tests/fp8_block_ref.py, fixture tests/golden/fp8_block.npz).

K_FLOOR and EQUAL are the project's constants for the same instruction at unit scales (K_FLOOR_GROUPED["fp8"], EQUAL_FP8):
conditions, not targets; what the kernels measure against them is in the comment above the constants."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_block_ref as R  # noqa: E402
from _parity import Guarded, check, k_needed, oracle_round  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "fp8_block.npz"))
with open(os.path.join(os.path.dirname(HERE), "include", "ao_mi355.h")) as fh:
    SEAM = int(re.search(r"#define AO_FP8_BLOCK_STREAM_MAX_ROWS (\d+)", fh.read()).group(1))  # the stream form up to these rows
# Measured on an MI355X over every Gaussian case below (profiles/pytest_gpu_fp8_block.log; each case prints its figures before it asserts):
#   stream form: worst k_needed 31 at (192, 130, 256) -- 24 at (129, 257, 384), 21 at (64, 130, 256), 20 at (16, 384, 128), at most 8
#                elsewhere; lowest equal fraction 0.9867 at (64, 130, 256)
#   tiled form:  worst k_needed 45 at (300, 128, 128) -- 23 at (193, 17, 128), 21 at (64, 130, 256) forced, 12 at (193, 384, 1152);
#                lowest equal fraction 0.9867 at (64, 130, 256) forced, 0.9884 on its own route
# Forced onto one shape the two forms give the same figures.  The equal fraction is asserted from 1024 elements on (_parity.check): the
# two smaller cases, (1, 128, 128) at 1.0000 and (1, 17, 256) at 0.9412 = 16 of 17, are printed only.  Both caps are far from binding.
K_FLOOR = 896
EQUAL = 0.95
STREAM, TILE = "fp8_block_stream_kernel", "fp8_block_tile_kernel"
CASES = [(1, 128, 128), (1, 17, 256), (15, 130, 1152), (16, 384, 128), (17, 257, 1152), (32, 128, 2304), (33, 384, 1152), (SEAM, 130, 256),
         (SEAM + 1, 17, 128), (SEAM + 1, 384, 1152), (129, 257, 384), (300, 128, 128)]
FORCED = [(17, 257, 1152), (64, 130, 256)]


def _dev():
    return torch.device("cuda", 0)


def _bf16(bits_np):
    return torch.from_numpy(np.ascontiguousarray(bits_np).astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16).to(_dev())


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _np(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _same_bf16(a, b):
    nan = lambda v: (v & 0x7FFF) > 0x7F80  # noqa: E731
    return np.array_equal(nan(a), nan(b)) and np.array_equal(np.where(nan(a), 0, a), np.where(nan(b), 0, b))


# ---- casts -------------------------------------------------------------------------------------------------------------------------
def test_weight_cast_equals_the_fixture():
    from ao_amd import ops

    q, s = ops.fp8_quantize_block_128x128(_bf16(GOLDEN["w"]))
    assert q.dtype == torch.float8_e4m3fn and tuple(s.shape) == (2, 3)
    assert R.same_codes(_np(q), GOLDEN["w_q"])
    np.testing.assert_array_equal(s.cpu().numpy(), GOLDEN["w_s"])


@pytest.mark.parametrize("name", ["seeded", "edge", "x3d"])
def test_activation_cast_equals_the_fixture(name):
    from ao_amd import ops

    x = GOLDEN[f"{name}_x"]
    q, s = ops.fp8_quantize_block_1x128(_bf16(x))
    assert tuple(q.shape) == x.shape and tuple(s.shape) == GOLDEN[f"{name}_s"].shape
    assert R.same_codes(_np(q), GOLDEN[f"{name}_q"])
    np.testing.assert_array_equal(s.cpu().numpy(), GOLDEN[f"{name}_s"])


def test_activation_cast_exhaustive():
    """Every finite bf16 value beside a fixed block amax (several amax values) equals fp8_block_ref's bytes."""
    from ao_amd import ops

    allb = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    vals = allb[(allb & 0x7F80) != 0x7F80]
    pad = (-len(vals)) % 127
    vals = np.concatenate([vals, np.zeros(pad, dtype=np.uint16)]).reshape(-1, 127)
    for amax in (448.0, 1.0, 5.0, 448.0 * 2.0 ** 40, 3.0 * 2.0 ** -100, 2.0 ** 120, 2.0 ** -130):
        ab = (np.array([amax], dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)
        x = np.concatenate([np.full((vals.shape[0], 1), ab[0], dtype=np.uint16), vals], axis=1)
        q, s = ops.fp8_quantize_block_1x128(_bf16(x))
        rq, rs = R.cast_1x128(x)
        np.testing.assert_array_equal(s.cpu().numpy(), rs, err_msg=f"amax {amax}")
        assert R.same_codes(_np(q), rq), f"amax {amax}"


@pytest.mark.parametrize("N", [128, 256, 384])
@pytest.mark.parametrize("K", [128, 256, 384])
def test_weight_cast_sweep(N, K):
    from ao_amd import ops

    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-6, 3, (N, 1), generator=g).float())).to(torch.bfloat16)
    w[127, 127] = -77.0       # the amax of the first block sits in its last row and column
    w[N - 1, K - 1] = 1000.0  # and of the last one (the same element at N = K = 128)
    q, s = ops.fp8_quantize_block_128x128(w.to(_dev()))
    rq, rs = R.cast_128x128(_bits(w))
    np.testing.assert_array_equal(s.cpu().numpy(), rs)
    assert R.same_codes(_np(q), rq)
    assert rs[-1, -1] == np.float32(torch.tensor(1000.0 / 448.0).to(torch.bfloat16).float().item())


# ---- the GEMM ----------------------------------------------------------------------------------------------------------------------
def _run_codes(aq, a_s, wq, ws, bias, M, N):
    from ao_amd import ops

    buf = Guarded(M, N, torch.bfloat16, _dev())
    ops.fp8_block_mm(_t(aq).view(torch.float8_e4m3fn), _t(a_s), _t(wq).view(torch.float8_e4m3fn), _t(ws), bias, out=buf.out)
    torch.cuda.synchronize()
    return buf


def _exact_operands(M, N, K, seed):
    """Integer e4m3 codes |q| <= 15, power-of-two scales that differ per (row, kb) and per (nb, kb) within 2^7 of one another: every
    partial sum, in any order, is exact in fp32 (asserted below), so the output bits are the chain's whatever the kernel's order."""
    from oracle import fp8_ref

    g = np.random.default_rng(seed)
    kb, nb = K // 128, (N + 127) // 128
    aq = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (M, K)).astype(np.float32))
    wq = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (N, K)).astype(np.float32))
    a_s = np.exp2(g.integers(-2, 2, (M, kb))).astype(np.float32)
    ws = np.exp2(g.integers(-2, 3, (nb, kb))).astype(np.float32)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(seed)) * 64).to(torch.bfloat16)
    y, S = R.linear_f64(aq, a_s, wq, ws)
    assert S.max() / 2.0 ** -4 < 2.0 ** 24, "the sums of this case are not exact in fp32 in every order"
    assert a_s.max() * ws.max() / (a_s.min() * ws.min()) <= 2.0 ** 7
    return aq, a_s, wq, ws, bias


def _exact_case(M, N, K, want):
    from ao_amd import ops

    assert ops.fp8_block_linear_kernel_name(M, N, K) == want
    aq, a_s, wq, ws, bias = _exact_operands(M, N, K, 1000 + M + N + K)
    for b in (None, bias):
        buf = _run_codes(aq, a_s, wq, ws, b.to(_dev()) if b is not None else None, M, N)
        ref = R.chain_bits(aq, a_s, wq, ws, _bits(b) if b is not None else None)
        check(buf, ref_bits=_t(ref.view(np.int16)))
    return len(np.unique(ref))


@pytest.mark.parametrize("M,N,K", CASES)
def test_exact_sums_pin_every_scale_index(M, N, K):
    distinct = _exact_case(M, N, K, STREAM if M <= SEAM else TILE)
    assert distinct > min(M * N, 64) // 2  # the outputs tell the elements apart


@pytest.mark.parametrize("form,want", [(1, STREAM), (2, TILE)])
@pytest.mark.parametrize("M,N,K", FORCED)
def test_exact_sums_with_each_form_forced(form, want, M, N, K):
    from ao_amd import ops

    try:
        ops.fp8_block_linear_set_form(form)
        _exact_case(M, N, K, want)
    finally:
        ops.fp8_block_linear_set_form(0)
    assert ops.fp8_block_linear_kernel_name(M, N, K) == (STREAM if M <= SEAM else TILE)


# The (m-tiles, waves) instances of the stream form that no case above launches.  One column tile (N = 16) asks for the most waves, the
# K / 128 k steps cap them; M = 1 / 17 / 33 rows take 1 / 2 / 4 m-tiles.
@pytest.mark.parametrize("M,K,pair", [(1, 512, (1, 4)), (17, 128, (2, 1)), (17, 256, (2, 2)), (17, 512, (2, 4)), (33, 512, (4, 4))],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_exact_sums_on_the_remaining_stream_instances(M, K, pair):
    from ao_amd import ops

    try:
        ops.fp8_block_linear_set_form(1)
        route = ops.fp8_block_linear_route(M, 16, K)
        assert (route["m_tiles"], route["waves"]) == pair
        _exact_case(M, 16, K, STREAM)
    finally:
        ops.fp8_block_linear_set_form(0)


def _operands(M, N, K, seed, bias):
    """The operand recipe of test_mx_linear_gpu._operands."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    b = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16) if bias else None
    return x.to(_dev()), w.to(_dev()), (b.to(_dev()) if b is not None else None)


def _cast_weight(w):
    """Our 128 x 128 cast of a weight of any N: rows padded with zeros to a multiple of 128 (they join no amax), the first N rows kept."""
    from ao_amd import ops

    N, K = w.shape
    pad = (-N) % 128
    wp = torch.cat([w, w.new_zeros(pad, K)]) if pad else w
    q, s = ops.fp8_quantize_block_128x128(wp)
    return q[:N].contiguous(), s


def _gaussian_case(M, N, K):
    from ao_amd import ops

    x, w, bias = _operands(M, N, K, 100 + M + N + K, True)
    aq, a_s = ops.fp8_quantize_block_1x128(x)
    wq, ws = _cast_weight(w)
    y64, S = R.linear_f64(_np(aq), a_s.cpu().numpy(), _np(wq), ws.cpu().numpy())
    ref64, S = _t(y64), _t(S)
    buf = Guarded(M, N, torch.bfloat16, _dev())
    ops.fp8_block_mm(aq, a_s, wq, ws, None, out=buf.out)
    torch.cuda.synchronize()
    eq = (buf.out == oracle_round(ref64, torch.bfloat16)).double().mean().item()
    print(f"fp8_block {ops.fp8_block_linear_kernel_name(M, N, K)} M={M} N={N} K={K}: k_needed {k_needed(buf.out, ref64, S, torch.bfloat16):.0f} equal {eq:.4f}")
    check(buf, ref64=ref64, S=S, K=K, k_floor=K_FLOOR, equal=EQUAL)
    # with a bias the launch must give bf16(f32(y_nobias) + f32(bias)) bit for bit: the launch is deterministic
    withb = Guarded(M, N, torch.bfloat16, _dev())
    ops.fp8_block_mm(aq, a_s, wq, ws, bias, out=withb.out)
    torch.cuda.synchronize()
    check(withb, ref_bits=_t(R.add_bias_bits(_bits(buf.out), _bits(bias)).view(np.int16)))


@pytest.mark.parametrize("M,N,K", CASES + [(8, 256, 7168)])
def test_gaussian_against_float64(M, N, K):
    from ao_amd import ops

    assert ops.fp8_block_linear_kernel_name(M, N, K) == (STREAM if M <= SEAM else TILE)
    _gaussian_case(M, N, K)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("M,N,K", FORCED)
def test_gaussian_with_each_form_forced(form, M, N, K):
    from ao_amd import ops

    try:
        ops.fp8_block_linear_set_form(form)
        assert ops.fp8_block_linear_kernel_name(M, N, K) == (STREAM if form == 1 else TILE)
        _gaussian_case(M, N, K)
    finally:
        ops.fp8_block_linear_set_form(0)


@pytest.mark.parametrize("M,N,K", [(1, 130, 256), (5, 128, 7168), (24, 257, 1152), (SEAM, 17, 128)])
def test_fused_cast_bitwise_equals_cast_then_gemm(M, N, K):
    from ao_amd import _lib, ops

    assert _lib.lib().ao_fp8_block_dynamic_linear_fits(M, N, K) == 1
    x, w, bias = _operands(M, N, K, 7 + M, True)
    x[0, :128] = x[0, :128] * 1e30  # a block that saturates beside a normal one
    wq, ws = _cast_weight(w)
    fused, two = Guarded(M, N, torch.bfloat16, _dev()), Guarded(M, N, torch.bfloat16, _dev())
    ops.fp8_block_linear(x, wq, ws, bias, fuse=True, out=fused.out)
    ops.fp8_block_linear(x, wq, ws, bias, fuse=False, out=two.out)
    torch.cuda.synchronize()
    assert not fused.guard_problems() and not two.guard_problems()
    assert not bool((fused.bits() == fused.sentinel).any())
    assert torch.equal(fused.raw, two.raw)
    # and the host rule's own choice gives the same bits
    assert torch.equal(ops.fp8_block_linear(x, wq, ws, bias).view(torch.int16), two.out.view(torch.int16))


def test_lane_map_one_hot():
    """One-hot operands at M = N = 16, K = 256: out[m][n] = a[m][k_m] b[n][k_m] a_s[m][kb] b_s[0][kb] picks the single k where row m is
    non-zero; distinct values per (row, k), two a_s per row and two b_s pin which lane and byte feeds which row, k and scale."""
    from oracle import fp8_ref

    M = N = 16
    K = 256
    a = np.zeros((M, K), dtype=np.float32)
    b = np.zeros((N, K), dtype=np.float32)
    for m in range(M):
        a[m, (37 * m + 5) % K] = 1 + (m % 7)
    for n in range(N):
        for m in range(M):
            if (m + n) % 5 == 0:
                b[n, (37 * m + 5) % K] = (1 + (n % 3)) * (-1 if m % 2 else 1)
    aq, wq = fp8_ref.f32_to_e4m3(a), fp8_ref.f32_to_e4m3(b)
    a_s = np.stack([np.exp2(np.arange(M) % 3), np.exp2(-(np.arange(M) % 2) - 1.0)], axis=1).astype(np.float32)
    ws = np.array([[0.5, 4.0]], dtype=np.float32)
    assert len({(37 * m + 5) % K // 128 for m in range(M)}) == 2
    buf = _run_codes(aq, a_s, wq, ws, None, M, N)
    y, _ = R.linear_f64(aq, a_s, wq, ws)
    assert torch.equal(buf.out.to(torch.float64).cpu(), torch.from_numpy(y))
    assert float(np.abs(y).sum()) > 0


# ---- quantize_ and the subclass ------------------------------------------------------------------------------------------------------
def _sqnr(ref, y):
    ref, y = ref.float(), y.float()
    return (20 * torch.log10(torch.linalg.norm(ref) / torch.linalg.norm(ref - y))).item()


def _config():
    from ao_amd.quantization import Float8DynamicActivationFloat8WeightConfig, PerBlock

    return Float8DynamicActivationFloat8WeightConfig(granularity=[PerBlock([1, 128]), PerBlock([128, 128])])


@pytest.mark.parametrize("bias_on", [False, True])
def test_quantize_mlp(bias_on):
    import torch.nn.functional as F

    from ao_amd.quantization import Float8Tensor, quantize_

    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(256, 384, bias=bias_on), torch.nn.ReLU(), torch.nn.Linear(384, 128, bias=bias_on))
    m = m.to(torch.bfloat16).to(_dev())
    x = torch.randn(9, 256, dtype=torch.bfloat16, device=_dev())
    with torch.no_grad():
        ref = m(x)
    quantize_(m, _config())
    w = m[0].weight
    assert isinstance(w, Float8Tensor) and w.shape == (384, 256) and list(w.block_size) == [128, 128] and tuple(w.scale.shape) == (3, 2)
    assert isinstance(m[2].weight, Float8Tensor) and tuple(m[2].weight.scale.shape) == (1, 3)
    with torch.no_grad():
        y = m(x)
        y0 = F.linear(x, w)
        y0b = m[0](x)
    assert y.dtype == torch.bfloat16 and _sqnr(ref, y) >= 25.0
    # the first linear against fp8_block_ref: the float64 sum of the reference's own codes within the parity bound
    aq, a_s = R.cast_1x128(_bits(x))
    wq, ws = _np(w.qdata), w.scale.cpu().numpy()
    ref64, S = R.linear_f64(aq, a_s, wq, ws)
    buf = Guarded(9, 384, torch.bfloat16, _dev())
    buf.out.copy_(y0)
    check(buf, ref64=_t(ref64), S=_t(S), K=256, k_floor=K_FLOOR, equal=EQUAL)
    if bias_on:
        np.testing.assert_array_equal(_bits(y0b), R.add_bias_bits(_bits(y0), _bits(m[0].bias.detach())))
    else:
        assert torch.equal(y0b.view(torch.int16), y0.view(torch.int16))
    # 3-D activations and an empty batch
    with torch.no_grad():
        assert torch.equal(m[0](x.reshape(3, 3, 256)).view(torch.int16), y0b.reshape(3, 3, 384).view(torch.int16))
        assert tuple(m[0](x[:0]).shape) == (0, 384)


def test_from_hp_weight_is_the_reference_cast():
    from ao_amd.quantization import Float8Tensor, PerBlock

    w = Float8Tensor.from_hp(_bf16(GOLDEN["w"]), granularity=PerBlock([128, 128]))
    assert list(w.block_size) == [128, 128] and tuple(w.scale.shape) == (2, 3)
    assert R.same_codes(_np(w.qdata), GOLDEN["w_q"])
    assert _same_bf16(_bits(w.dequantize()), GOLDEN["w_dequant"])
    s = w[128:256, 128:384]
    np.testing.assert_array_equal(_np(s.qdata), GOLDEN["w_slice_q"])
    np.testing.assert_array_equal(s.scale.cpu().numpy(), GOLDEN["w_slice_s"])
    assert _same_bf16(_bits(s.dequantize()), GOLDEN["w_slice_dequant"])
    a = Float8Tensor.from_hp(_bf16(GOLDEN["x3d_x"]), granularity=PerBlock([1, 128]))
    assert list(a.block_size) == [1, 1, 128] and R.same_codes(_np(a.qdata), GOLDEN["x3d_q"])
    with pytest.raises(AssertionError, match=r"\(200, 384\)"):
        Float8Tensor.from_hp(torch.zeros(200, 384, dtype=torch.bfloat16, device=_dev()), granularity=PerBlock([128, 128]))


def test_raw_checkpoint_tensors_run_like_from_hp():
    """Float8Tensor(weight, weight_scale_inv, [128, 128], ...) built directly, as a checkpoint loader does -- also with an N that is no
    multiple of 128 -- gives the output of the from_hp tensor; act_pre_scale is honoured; t() and a slice of K run."""
    import torch.nn.functional as F

    from ao_amd.quantization import Float8Tensor, PerBlock, QuantizeTensorToFloat8Kwargs

    x, w, bias = _operands(9, 256, 384, 11, True)
    kw = QuantizeTensorToFloat8Kwargs(granularity=PerBlock([1, 128]))
    hp = Float8Tensor.from_hp(w, granularity=PerBlock([128, 128]), act_quant_kwargs=kw)
    raw = Float8Tensor(hp.qdata.clone(), hp.scale.clone(), [128, 128], torch.bfloat16, kw)
    y = F.linear(x, hp, bias)
    assert torch.equal(F.linear(x, raw, bias).view(torch.int16), y.view(torch.int16))
    ragged = Float8Tensor(hp.qdata[:130].contiguous(), hp.scale.clone(), [128, 128], torch.bfloat16, kw)
    assert torch.equal(F.linear(x, ragged, bias[:130]).view(torch.int16), y[:, :130].view(torch.int16))
    assert torch.equal(torch.mm(x, hp.t()).view(torch.int16), F.linear(x, hp).view(torch.int16))
    pre = torch.full((384,), 0.5, dtype=torch.bfloat16, device=_dev())
    scaled = Float8Tensor(hp.qdata, hp.scale, [128, 128], torch.bfloat16, kw, pre)
    assert torch.equal(F.linear(x, scaled).view(torch.int16), F.linear(x * pre, hp).view(torch.int16))
    part = hp[:, 128:384]
    assert torch.equal(F.linear(x[:, 128:384].contiguous(), part).view(torch.int16),
                       F.linear(x[:, 128:384].contiguous(), Float8Tensor(hp.qdata[:, 128:384].contiguous(), hp.scale[:, 1:3].contiguous(),
                                                                         [128, 128], torch.bfloat16, kw)).view(torch.int16))


def test_torch_compile_fullgraph_bitwise():
    from ao_amd.quantization import quantize_

    torch.manual_seed(5)
    lin = torch.nn.Linear(256, 128, bias=True).to(torch.bfloat16).to(_dev())
    quantize_(lin, _config())
    x = torch.randn(3, 256, dtype=torch.bfloat16, device=_dev())
    with torch.no_grad():
        eager = lin(x)
        compiled = torch.compile(lin, fullgraph=True)(x)
    assert torch.equal(eager.view(torch.int16), compiled.view(torch.int16))


def test_refusals_name_blockwise():
    import torch.nn.functional as F

    from ao_amd.quantization import Float8Tensor, PerBlock, QuantizeTensorToFloat8Kwargs

    kw = QuantizeTensorToFloat8Kwargs(granularity=PerBlock([1, 128]))
    w = Float8Tensor.from_hp(torch.randn(256, 256, dtype=torch.bfloat16, device=_dev()), granularity=PerBlock([128, 128]), act_quant_kwargs=kw)
    x = torch.randn(2, 256, dtype=torch.bfloat16, device=_dev())
    for call in (lambda: torch.cat([w, w]), lambda: torch.split(w, 128), lambda: F.linear(x.float(), w), lambda: F.linear(x.half(), w),
                 lambda: F.linear(x, Float8Tensor(w.qdata, w.scale, [128, 128], torch.bfloat16)), lambda: w[0:64],
                 lambda: Float8Tensor.from_hp(torch.randn(2, 128, 128, dtype=torch.bfloat16, device=_dev()), granularity=PerBlock([128, 128]))):
        with pytest.raises(NotImplementedError, match="blockwise"):
            call()
