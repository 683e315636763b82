"""Intx on the GPU: the casts byte for byte against the numpy restatement (tests/intx_ref.py, which reproduces the reference's recorded bytes),
the pack / unpack pair over the full code range, and the linear in both forms and from both layouts against the float64 product of the
decoded operands -- bit for bit where every partial sum is exact in fp32, inside the fp32-accumulation bound on Gaussian operands."""
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import intx_ref as R
from ao_amd import ops
from ao_amd.prototype import IntxBitPackedTensor
from ao_amd.quantization import (Int8DynamicActivationIntxWeightConfig, IntxUnpackedToInt8Tensor, IntxWeightOnlyConfig, MappingType, PerAxis,
                                 PerGroup, quantize_)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intx.npz"))
SEAM = 64  # AO_INTX_LINEAR_STREAM_MAX_M


def bf(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).to(DEV)


def bits(t):
    """bf16 tensor -> uint16 patterns, every NaN as intx_ref.NAN_BITS"""
    b = t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).copy()
    b[torch.isnan(t).cpu().numpy()] = R.NAN_BITS
    return b


@pytest.mark.parametrize("mapping", R.MAPPINGS)
@pytest.mark.parametrize("b", range(1, 9))
def test_quantize_byte_for_byte(b, mapping):
    edge = np.random.default_rng(b).standard_normal((17, 320)).astype(np.float32)
    edge[3, 64:128] = 0
    cases = [(GOLDEN["w"], g) for g in (32, 128, 256)] + [(R.bf16.to_bits(R.bf16.bf16_round(edge)), g) for g in (32, 64, 320)]
    for w, g in cases:
        q, s, zp = ops.intx_quantize(bf(w), g, b, mapping)
        rq, rs, rzp = R.from_hp(w, b, mapping, g)
        assert np.array_equal(bits(s), rs) and np.array_equal(zp.cpu().numpy(), rzp) and np.array_equal(q.cpu().numpy(), rq), (w.shape, g)
        again = ops.intx_quantize(bf(w), g, b, mapping, s, zp)[0]  # the custom scale / zero-point branch: quantize_affine alone
        assert torch.equal(again, q)


@pytest.mark.parametrize("k", [256, 4096])
@pytest.mark.parametrize("m", [1, 5, 64])
def test_act_fake_quant_byte_for_byte(m, k):
    x = np.random.default_rng(m * k).standard_normal((m, k)).astype(np.float32) * 3
    x[0, 0] = 17.0
    if m > 1:
        x[1], x[2], x[3] = 0.3125, 0.0, -np.abs(x[3]) - 1
    xb = R.bf16.to_bits(R.bf16.bf16_round(x))
    assert np.array_equal(bits(ops.int8_fake_quantize_per_token_asym(bf(xb))), R.act_fake_quant(xb))


@pytest.mark.parametrize("b", range(1, 8))
def test_pack_unpack_and_dequantize(b):
    qmin, qmax = R.bounds(b)
    rng = np.random.default_rng(b)
    q = rng.integers(qmin, qmax + 1, size=(17, 320)).astype(np.int8)
    q[0, :1 << b] = np.arange(qmin, qmax + 1)[:320]
    s = R.bf16.to_bits(R.bf16.bf16_round(rng.uniform(0.01, 2, size=(17, 5)).astype(np.float32)))
    zp = rng.integers(qmin, qmax + 1, size=(17, 5)).astype(np.int8)
    tq, ts, tz = torch.from_numpy(q).to(DEV), bf(s), torch.from_numpy(zp).to(DEV)
    packed = ops.intx_pack(tq, b)
    assert packed.shape == (17, 10 * b) and np.array_equal(packed.cpu().numpy(), R.pack(q, b))
    assert torch.equal(ops.intx_unpack(packed, b), tq)
    u = IntxUnpackedToInt8Tensor(tq, ts, tz, getattr(torch, f"int{b}"), (1, 64), torch.bfloat16, None)
    p = IntxBitPackedTensor.from_intx_unpacked_to_int8_tensor(u)
    back = p.to_intx_unpacked_to_int8_tensor()
    assert torch.equal(back.qdata, tq) and torch.equal(back.scale, ts) and torch.equal(back.zero_point, tz) and back.block_size == (1, 64)
    want = R.dequantize(q, s, zp)
    assert np.array_equal(bits(u.dequantize()), want) and np.array_equal(bits(p.dequantize()), want)


def _operands(b, m, n, k, g, gen, exact):
    """x, codes, scale, zero_point and the decoded weight.  exact: small-integer x, power-of-two scales, zero-points at both extremes, so every
    partial sum is exact in fp32."""
    qmin, qmax = R.bounds(b)
    q = torch.randint(qmin, qmax + 1, (n, k), generator=gen, device=DEV, dtype=torch.int32).to(torch.int8)
    q[0, :2] = torch.tensor([qmin, qmax], dtype=torch.int8)
    if exact:
        x = torch.randint(-4, 5, (m, k), generator=gen, device=DEV).to(torch.bfloat16)
        s = torch.pow(2.0, torch.randint(-2, 2, (n, k // g), generator=gen, device=DEV).float()).to(torch.bfloat16)
        zp = torch.where(torch.rand((n, k // g), generator=gen, device=DEV) < 0.5, qmin, qmax).to(torch.int8)
    else:
        x = torch.randn((m, k), generator=gen, device=DEV).to(torch.bfloat16)
        s = (torch.rand((n, k // g), generator=gen, device=DEV) * 0.1 + 0.01).to(torch.bfloat16)
        zp = torch.randint(qmin, qmax + 1, (n, k // g), generator=gen, device=DEV, dtype=torch.int32).to(torch.int8)
    w = ((q.double().view(n, k // g, g) - zp.double()[..., None]) * s.double()[..., None]).float().to(torch.bfloat16).view(n, k)
    return x, q, s, zp, w


@pytest.fixture
def form(request):
    ops.intx_linear_set_form(request.param)
    yield request.param
    ops.intx_linear_set_form(0)


@pytest.mark.parametrize("form", [1, 2], indirect=True)
@pytest.mark.parametrize("b", [1, 3, 4, 7, 8])
def test_linear_exact_sums_bit_for_bit(b, form):
    gen = torch.Generator(device=DEV).manual_seed(100 * b + form)
    for m in (1, 3, 16, 17, SEAM, SEAM + 1, 65):
        for n in (16, 40):
            for k in (256, 320):
                for g in (32, 64, k):
                    x, q, s, zp, w = _operands(b, m, n, k, g, gen, exact=True)
                    bias = (torch.randint(-8, 9, (n,), generator=gen, device=DEV).float() / 4).to(torch.bfloat16)
                    packed = ops.intx_pack(q, b)
                    for bb in (None, bias):
                        ref = x.double() @ w.double().T + (0 if bb is None else bb.double())
                        ref = ref.float().to(torch.bfloat16)  # (the sums are integers over 4 below 2^22: the float step is exact)
                        for codes in (q, packed):
                            out = ops.intx_linear(x, codes, s, zp, b, bb)
                            assert torch.equal(out, ref), (m, n, k, g, bb is not None, codes.dtype, (out.float() - ref.float()).abs().max().item())


@pytest.mark.parametrize("form", [1, 2], indirect=True)
@pytest.mark.parametrize("b,m,n,k,g", [(3, 17, 40, 320, 64), (8, 65, 40, 320, 32), (5, 1, 16, 4096, 128), (2, 64, 72, 1024, 1024), (6, 130, 200, 512, 64)])
def test_linear_gaussian_inside_the_fp32_bound(b, m, n, k, g, form):
    gen = torch.Generator(device=DEV).manual_seed(b * m)
    x, q, s, zp, w = _operands(b, m, n, k, g, gen, exact=False)
    ref = x.double() @ w.double().T
    bound = ref.abs() * 2.0 ** -8 + k * 2.0 ** -24 * (x.double().abs() @ w.double().abs().T)
    for codes in (q, ops.intx_pack(q, b)):
        err = (ops.intx_linear(x, codes, s, zp, b).double() - ref).abs()
        print(f"b={b} m={m} form={form} {codes.dtype}: max err / bound = {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all())


def _exact_model(gen):
    """Two linears whose int4 ASYMMETRIC quantization is exact: weights on the 1/4 grid, every group reaching -2 and 1.75 (scale 1/4, zero 0)."""
    model = torch.nn.Sequential(torch.nn.Linear(256, 64, dtype=torch.bfloat16), torch.nn.Linear(64, 24, bias=False, dtype=torch.bfloat16)).to(DEV)
    for lin in model:
        w = torch.randint(-8, 8, lin.weight.shape, generator=gen, device=DEV).float() / 4
        w[:, 0::32], w[:, 1::32] = -2.0, 1.75
        lin.weight.data.copy_(w)
        if lin.bias is not None:
            lin.bias.data.copy_(torch.randint(-8, 9, lin.bias.shape, generator=gen, device=DEV).float() / 4)
    return model


@pytest.mark.parametrize("dynamic", [False, True])
def test_quantize_end_to_end(dynamic):
    gen = torch.Generator(device=DEV).manual_seed(7)
    make = ((lambda fmt: Int8DynamicActivationIntxWeightConfig(torch.int4, PerGroup(32), MappingType.ASYMMETRIC, intx_packing_format=fmt)) if dynamic
            else (lambda fmt: IntxWeightOnlyConfig(torch.int4, PerGroup(32), MappingType.ASYMMETRIC, intx_packing_format=fmt)))
    ref_model = _exact_model(gen)
    unpacked, packed = _exact_model(gen), _exact_model(gen)
    unpacked.load_state_dict(ref_model.state_dict()), packed.load_state_dict(ref_model.state_dict())
    quantize_(unpacked, make("unpacked_to_int8"))
    quantize_(packed, make("bit_packed"))
    assert "IntxUnpackedToInt8Tensor" in repr(unpacked[0]) and isinstance(packed[1].weight, IntxBitPackedTensor)
    for i, lin in enumerate(ref_model):
        k = lin.in_features
        for m in (1, 5, 70):
            # integers in [-128, 127] reaching both ends: the per-token int8 quantization (scale 1, zero 0) returns them unchanged
            x = torch.randint(-128, 128, (m, k), generator=gen, device=DEV).float()
            x[:, 0], x[:, 1] = -128, 127
            x = x.to(torch.bfloat16)
            wu, wp = unpacked[i].weight, packed[i].weight
            assert torch.equal(wu.dequantize(), lin.weight) and torch.equal(wp.dequantize(), lin.weight)
            x_fq = ops.int8_fake_quantize_per_token_asym(x) if dynamic else x
            assert torch.equal(x_fq, x)
            want = F.linear(x_fq, wu.dequantize(), lin.bias)
            got_u, got_p = unpacked[i](x), packed[i](x)
            assert torch.equal(got_u, want) and torch.equal(got_p, got_u), (i, m)
    # a captured decode call replays to the eager bytes
    x = torch.randint(-4, 5, (1, 256), generator=gen, device=DEV).to(torch.bfloat16)
    x[0, 0], x[0, 1] = -128, 127
    eager = packed(x)
    static_x = x.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = packed(static_x)
    for _ in range(3):
        static_y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_y, eager)
    # both tensors round-trip through torch.save / torch.load(weights_only=True)
    for model in (unpacked, packed):
        buf = io.BytesIO()
        torch.save(model.state_dict(), buf)
        buf.seek(0)
        state = torch.load(buf, weights_only=True)
        w = state["0.weight"]
        assert type(w) is type(model[0].weight) and w.target_dtype == torch.int4 and tuple(w.block_size) == (1, 32)
        assert w.activation_quantization == model[0].weight.activation_quantization
        assert torch.equal(w.dequantize(), model[0].weight.dequantize())
