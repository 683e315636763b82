"""BitNet b1.58 on the GPU, byte for byte against tests/bitnet_ref.py: the casts, both forms of the matmul at every edge of their tiles, the
training and inference modules end to end, and one graph capture.  The sums are exact, so nothing here has a tolerance but the abs-mean."""
import copy
import functools

import numpy as np
import pytest
import torch

import bitnet_ref as R
from ao_amd import ops
from ao_amd.prototype import quantized_training as Q
from ao_amd.quantization import quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"


def gpu(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to(DEV)


@pytest.mark.parametrize("scale", [0.5, 3e-6])  # 3e-6: below the 1e-5 clip
@pytest.mark.parametrize("N,K", [(1, 4), (3, 64), (17, 260), (130, 1024)])
def test_weight_cast_bytes(N, K, scale):
    gen = torch.Generator().manual_seed(N * K)
    s = max(scale, 1e-5)
    w = (torch.randn(N, K, generator=gen) * s).to(torch.bfloat16)
    ties = torch.tensor([0.5, -0.5, 1.5, -1.5, -0.0, 2.5, -2.5, 0.0]) * (0.5 if scale == 0.5 else 0.0)  # exact quotients under scale 0.5
    if scale == 0.5:
        w.view(-1)[: min(8, N * K)] = ties[: min(8, N * K)].to(torch.bfloat16)
    want_q, want_packed = R.quantize_weight(w, scale)
    packed, q8 = ops.bitnet_quantize_weight(gpu(w), torch.tensor(scale, dtype=torch.float32, device=DEV), with_int8=True)
    assert packed.shape == (N, K // 4) and packed.dtype == torch.int8
    assert np.array_equal(q8.cpu().numpy(), want_q) and np.array_equal(packed.cpu().numpy(), want_packed)
    assert np.array_equal(ops.bitnet_quantize_weight(gpu(w), torch.tensor(scale, dtype=torch.float32, device=DEV)).cpu().numpy(), want_packed)
    if scale == 0.5:
        assert want_q.reshape(-1)[: min(4, N * K)].tolist() == [0, 0, 1, -1][: min(4, N * K)]  # 0.5 and 1.5 round to even


@pytest.mark.parametrize("N,K", [(1, 4), (3, 64), (17, 260), (130, 1024)])
def test_dequantize_bytes(N, K):
    packed = torch.randint(-128, 128, (N, K // 4), generator=torch.Generator().manual_seed(K), dtype=torch.int8)  # field 2 (-2) included
    got = ops.bitnet_dequantize(gpu(packed))
    assert got.shape == (N, K) and got.dtype == torch.bfloat16
    assert torch.equal(R.bits(got.cpu()), R.bits(R.to_bf16(R.unpack(packed.numpy()))))


@pytest.mark.parametrize("K", [64, 320])
@pytest.mark.parametrize("M", [1, 5, 17])
def test_act_cast_bytes(M, K):
    x = (torch.randn(M, K, generator=torch.Generator().manual_seed(M + K)) * 3).to(torch.bfloat16)
    # row 0: amax 1.484375, whose quotient by 127 rounds DOWN to the bf16 scale 0.01165771484375: x * inv = 127.33, the largest overshoot of
    # 127 over every bf16 amax -- no finite row reaches 127.5, so the clip at -128 is dead code of the chain and the nearest case is this one.
    # The last row of M > 1: all zero (the eps path)
    x[0] = 0
    x[0, 1], x[0, 2], x[0, 3] = -1.484375, 1.484375, 1.4765625
    if M > 1:
        x[-1] = 0
    want_q, want_s = R.quantize_act(x)
    q, s = ops.bitnet_quantize_act(gpu(x))
    assert q.dtype == torch.int8 and s.dtype == torch.bfloat16 and s.shape == (M,)
    assert torch.equal(R.bits(s.cpu()), R.bits(want_s)) and np.array_equal(q.cpu().numpy(), want_q)
    assert want_q[0, 1] == -127 and (M == 1 or (want_s[-1] == 0 and not want_q[-1].any()))


@pytest.mark.parametrize("N,K", [(1, 4), (17, 260), (512, 1024)])
def test_absmean_within_one_ulp_and_reproducible(N, K):
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(N)).to(torch.bfloat16)
    mean64 = R.absmean64(w)
    a, a16 = ops.bitnet_absmean(gpu(w), with_bf16=True)
    b = Q.get_bitnet_scale(gpu(w))
    assert a.dtype == torch.float32 and a.shape == () and abs(float(a.cpu().double()) - mean64) <= 2.0 ** -23 * mean64
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(R.bits(a16.cpu()), R.bits(a.cpu().to(torch.bfloat16)))


@functools.lru_cache(maxsize=None)
def mm_case(M, N, K):
    """Operands in which a wrong row, column or field index changes the bits, and the two expected outputs (without / with bias)."""
    rng = np.random.default_rng(M * 7919 + N * 31 + K)
    a = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    a[0, 0] = -128
    q = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(N, K), p=[0.5, 0.3, 0.2])
    rs = R.to_bf16((np.arange(M, dtype=np.float32) + 1) / 256)  # distinct, exact in bf16 up to M = 256
    ts = R.to_bf16(np.float32(0.0371))
    bias = R.to_bf16(rng.standard_normal(N).astype(np.float32) * 40)
    return a, R.pack(q), rs, ts, bias, R.mm(a, q, rs, ts), R.mm(a, q, rs, ts, bias)


# M: both sides of the streaming seam (16) and of the tiled form's 128-row tile; N: 150 is no multiple of either form's tile (16, 64) nor of
# the 4-column store; K = 832: 13 steps of 64 (odd), and a streaming wave step (256 k) whose last lane groups are past the end
@pytest.mark.parametrize("form", [ops.BITNET_MM_STREAM, ops.BITNET_MM_TILED])
@pytest.mark.parametrize("K", [64, 192, 832])
@pytest.mark.parametrize("N", [16, 48, 150])
@pytest.mark.parametrize("M", [1, 7, 16, 17, 64, 127, 129])
def test_mm_bits(M, N, K, form):
    a, packed, rs, ts, bias, want, want_bias = mm_case(M, N, K)
    got = ops.bitnet_mm(gpu(a), gpu(packed), gpu(rs), gpu(ts), None, form)
    got_bias = ops.bitnet_mm(gpu(a), gpu(packed), gpu(rs), gpu(ts), gpu(bias), form)
    assert got.shape == (M, N) and torch.equal(R.bits(got.cpu()), R.bits(want)) and torch.equal(R.bits(got_bias.cpu()), R.bits(want_bias))


def test_mm_streams_more_than_one_lds_chunk():
    a, packed, rs, ts, bias, _, want_bias = mm_case(3, 40, 2048 + 448)
    assert torch.equal(R.bits(ops.bitnet_mm(gpu(a), gpu(packed), gpu(rs), gpu(ts), gpu(bias)).cpu()), R.bits(want_bias))


@pytest.fixture(scope="module")
def trained():
    torch.manual_seed(5)
    model = torch.nn.Sequential(torch.nn.Linear(64, 128, bias=True), torch.nn.Linear(128, 64, bias=False)).to(torch.bfloat16).to(DEV)
    plain = copy.deepcopy(model)
    quantize_(model, Q.BitNetTrainingConfig())
    return model, plain


@pytest.mark.parametrize("M", [1, 33])
def test_training_forward_and_inference_bits(trained, M):
    model, plain = trained
    x = torch.randn(M, 64, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16)
    want = x
    for lin in plain:  # the restated chain under the scale the kernel produced (read back here only)
        scale = ops.bitnet_absmean(lin.weight.detach()).item()
        want = R.linear(want, lin.weight.detach().cpu(), scale, None if lin.bias is None else lin.bias.detach().cpu())
    with torch.no_grad():
        got = model(gpu(x))
        frozen, refrozen = copy.deepcopy(plain), copy.deepcopy(plain)
        quantize_(frozen, Q.BitNetInferenceConfig())
        assert isinstance(frozen[0].weight, Q.BitNetPacked2bitLinearWeight) and not frozen[0].weight.requires_grad
        quantize_(refrozen, Q.BitNetTrainingConfig())  # a linear under training converts as well
        quantize_(refrozen, Q.BitNetInferenceConfig())
        assert torch.equal(R.bits(got.cpu()), R.bits(want))
        assert torch.equal(frozen(gpu(x)), got) and torch.equal(refrozen(gpu(x)), got)
        deq = frozen[1].weight.dequantize()
        assert torch.equal(deq, Q._unpack_i2_in_i8(frozen[1].weight.int_data).to(torch.bfloat16) * frozen[1].weight.scale)


def test_backward_is_the_reference_formulas(trained):
    model, _ = trained
    gen = torch.Generator().manual_seed(9)
    x = gpu(torch.randn(2, 9, 64, generator=gen).to(torch.bfloat16))
    g = gpu(torch.randn(2, 9, 64, generator=gen).to(torch.bfloat16))
    h = model[0](x)
    h.retain_grad()
    model[1](h).backward(g)
    w = model[1].weight._data
    scale, ts = ops.bitnet_absmean(w, with_bf16=True)
    w_i8 = Q.quantize_bitnet_weight(w, scale)
    assert torch.equal(Q._unpack_i2_in_i8(ops.bitnet_quantize_weight(w, scale)), w_i8)
    h_i8, rs = ops.bitnet_quantize_act(h.detach().reshape(-1, 128))
    g2 = g.reshape(-1, 64)
    assert torch.equal(h.grad, ((g2 @ w_i8.to(torch.bfloat16)) * ts).view(2, 9, 128))
    assert torch.equal(model[1].weight.grad, g2.T @ (h_i8 * rs.view(-1, 1)))
    assert model[0].bias.grad is not None and model[0].weight.grad.shape == (128, 64)


def test_graph_replays_give_the_eager_bytes(trained):
    model, _ = trained
    x = gpu(torch.randn(5, 64, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16))
    with torch.no_grad():
        eager = model(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # a host synchronisation on the path would fail the capture
            out = model(x)
        for _ in range(3):
            out.zero_()
            graph.replay()
            assert torch.equal(out, eager)
