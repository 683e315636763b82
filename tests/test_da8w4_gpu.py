"""W4A8 on the GPU against tests/da8w4_ref.py: casts byte for byte, the linear bit for bit (exact sums) and in its bound, quantize_, a graph."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import da8w4_ref as R
from ao_amd import ops
from ao_amd.prototype import Int4OpaqueTensor, Int8DynamicActivationInt4WeightConfig
from ao_amd.quantization import MappingType, quantize_

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "da8w4.npz"))


def dev(a):
    """a numpy array on the GPU; uint16 arrays are bf16 bit patterns"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16)).cuda().view(torch.bfloat16) if a.dtype == np.uint16 else torch.from_numpy(a).cuda()


def bits_of(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def round_bits(a):
    return R.bf16.to_bits(R.bf16.bf16_round(np.asarray(a).astype(np.float32)))


def check_weight_cast(w_bits, g):
    qw, sw, zw = R.weight_cast(w_bits, g)
    qdata, sz, qzeros, comp = ops.da8w4_quantize_weight(dev(w_bits), g)
    want_sz, want_qz, want_comp = R.weight_meta(qw, sw, zw)
    assert np.array_equal(qdata.cpu().numpy(), R.pack_weight(qw))
    assert np.array_equal(sz.cpu().numpy().view(np.uint32), want_sz.view(np.uint32))
    assert np.array_equal(qzeros.cpu().numpy(), want_qz) and np.array_equal(comp.cpu().numpy(), want_comp)
    want_dq = (qw.astype(np.float32) - np.repeat(zw, g, axis=1)) * np.repeat(sw, g, axis=1)  # exact in fp32; one rounding to bf16
    assert np.array_equal(bits_of(ops.da8w4_dequantize(qdata, sz, w_bits.shape[1])), round_bits(want_dq))


def check_act_cast(x_bits, g, symmetric):
    qa, sa, za = R.act_cast(x_bits, symmetric)
    want_codes, want_meta = R.act_device(qa, za, g, symmetric)
    q, s, zp, meta = ops.da8w4_quantize_act(dev(x_bits), g, symmetric)
    assert np.array_equal(q.cpu().numpy(), want_codes) and np.array_equal(meta.cpu().numpy(), want_meta)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), sa.view(np.uint32)) and np.array_equal(zp.cpu().numpy(), za)


@pytest.mark.parametrize("g", R.GROUPS)
def test_casts_match_the_restatement_byte_for_byte(g):
    """K in {g, 5 g}: {32, 160} at g = 32, the smallest K and one past a superblock with a padded tail; then the recorded grid"""
    rng = np.random.default_rng(g)
    for k in (g, 5 * g):
        check_weight_cast(round_bits(rng.standard_normal((32, k)) * 0.05), g)
        for m in (1, 17):
            for symmetric in (False, True):
                check_act_cast(round_bits(rng.standard_normal((m, k)) * 3), g, symmetric)
    for k in (g, 3 * g):
        check_weight_cast(GOLDEN["w"][:, :k], g)
    for symmetric in (False, True):
        check_act_cast(GOLDEN["x"], g, symmetric)


def exact_operands(rng, m, n, k, g, symmetric):  # small integer codes around random zero-points, power-of-two scales: every fp32 sum is exact
    za = np.zeros(m, np.int32) if symmetric else rng.integers(100, 150, m).astype(np.int32)
    qa = (za[:, None] + rng.integers(-3, 4, (m, k))).astype(np.int8 if symmetric else np.uint8)
    zw = rng.integers(0, 16, (n, k // g)).astype(np.int32)
    qw = np.clip(np.repeat(zw, g, axis=1) + rng.integers(-3, 4, (n, k)), 0, 15).astype(np.uint8)
    sa = (2.0 ** rng.integers(-3, 1, m)).astype(np.float32)
    sw = (2.0 ** rng.integers(-2, 2, (n, k // g))).astype(np.float32)
    return qa, sa, za, qw, sw, zw


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("g", R.GROUPS)
def test_linear_exact_sum_operands_bit_for_bit(g, form, symmetric, with_bias):
    rng = np.random.default_rng(1000 * g + 10 * form + 2 * symmetric + with_bias)
    try:
        ops.da8w4_linear_set_form(form)
        for n in R.LINEAR_N:
            for k in R.LINEAR_K[g]:
                qw, sw, zw = exact_operands(rng, 1, n, k, g, symmetric)[3:]
                packed, sz = dev(R.pack_weight(qw)), dev(R.weight_meta(qw, sw, zw)[0])
                bias = round_bits(rng.integers(-32, 33, n) / 4) if with_bias else None
                for m in R.LINEAR_M:
                    qa, sa, za = exact_operands(rng, m, n, k, g, symmetric)[:3]
                    codes, meta = R.act_device(qa, za, g, symmetric)
                    x = torch.empty((m, k), dtype=torch.bfloat16, device="cuda")  # (only its shape is read: the cast is given)
                    y = ops.da8w4_linear(x, packed, sz, None if bias is None else dev(bias), symmetric, act=(dev(codes), dev(sa), dev(meta)))
                    ref, _ = R.linear64(qa, sa, za, qw, sw, zw, bias)  # (an fp32 value held in float64: one rounding to bf16 is left)
                    assert np.array_equal(bits_of(y), round_bits(ref)), (m, n, k)
    finally:
        ops.da8w4_linear_set_form(0)


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("g", R.GROUPS)
def test_linear_gaussian_operands_inside_the_bound(g, form, symmetric):
    rng = np.random.default_rng(7 * g + form)
    m, n, k = 65, 96, 384 + g
    x_bits, w_bits, bias = (round_bits(rng.standard_normal(sh) * sc) for sh, sc in (((m, k), 3), ((n, k), 0.05), ((n,), 1)))
    qa, sa, za = R.act_cast(x_bits, symmetric)
    qw, sw, zw = R.weight_cast(w_bits, g)
    ref, mag = R.linear64(qa, sa, za, qw, sw, zw, bias)
    qdata, sz, _, _ = ops.da8w4_quantize_weight(dev(w_bits), g)
    try:
        ops.da8w4_linear_set_form(form)
        y = ops.da8w4_linear(dev(x_bits), qdata, sz, dev(bias), symmetric)
    finally:
        ops.da8w4_linear_set_form(0)
    ratio = np.abs(y.double().cpu().numpy() - ref) / R.bound(ref, mag, k // g)
    print(f"g={g} form={form} symmetric={symmetric}: max err / bound = {ratio.max():.3f}")
    assert np.all(ratio <= 1)


@pytest.mark.parametrize("mapping", [MappingType.ASYMMETRIC, MappingType.SYMMETRIC])
@torch.no_grad()
def test_quantize_toy_model_matches_ops_and_the_formats_own_error(mapping):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(160, 96, dtype=torch.bfloat16), torch.nn.Linear(96, 32, bias=False, dtype=torch.bfloat16)).cuda()
    x = torch.randn(3, 7, 160, device="cuda").to(torch.bfloat16)
    want = model(x).double().cpu().numpy().reshape(21, 32)
    weights, bias0 = [bits_of(layer.weight.detach()) for layer in model], bits_of(model[0].bias.detach())
    quantize_(model, Int8DynamicActivationInt4WeightConfig(group_size=32, act_mapping_type=mapping))
    symmetric = mapping == MappingType.SYMMETRIC
    assert all(isinstance(layer.weight, Int4OpaqueTensor) and layer.weight.act_mapping_type == mapping.name.lower() for layer in model)
    y = model(x)
    h = ops.da8w4_linear(x, model[0].weight.qdata, model[0].weight.scale_and_zero, model[0].bias, symmetric)
    assert y.shape == (3, 7, 32) and torch.equal(y, ops.da8w4_linear(h, model[1].weight.qdata, model[1].weight.scale_and_zero, None, symmetric))
    assert torch.equal(F.linear(x, model[0].weight, model[0].bias), h)
    # the same chain in float64, each layer's output rounded to bf16 as the activations between the layers are
    h64 = bits_of(x).reshape(21, 160)
    for w_bits, b in zip(weights, (bias0, None)):
        out64, _ = R.linear64(*R.act_cast(h64, symmetric), *R.weight_cast(w_bits, 32), b)
        h64 = round_bits(out64)
    got, chain = (10 * np.log10(np.sum(want ** 2) / np.sum((want - v) ** 2))
                  for v in (y.double().cpu().numpy().reshape(21, 32), R.bf16.from_bits(h64).astype(np.float64)))
    print(f"{mapping.name}: SQNR kernel {got:.3f} dB, float64 chain {chain:.3f} dB")
    assert abs(got - chain) <= 0.1


def test_graph_replays_give_the_eager_bytes():
    rng = np.random.default_rng(5)
    w = Int4OpaqueTensor.from_hp_da8w4(dev(round_bits(rng.standard_normal((96, 256)) * 0.05)), 64)
    xs = [dev(round_bits(rng.standard_normal((1, 256)) * 3)) for _ in range(3)]
    eager = [F.linear(x, w) for x in xs]
    static = xs[0].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        F.linear(static, w)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = F.linear(static, w)
    for x, want in zip(xs, eager):
        static.copy_(x)
        graph.replay()
        assert torch.equal(out, want)
