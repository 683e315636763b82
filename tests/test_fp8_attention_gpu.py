"""FP8 attention on the GPU: the cast byte for byte against the CPU chain, the kernel against float64 SDPA on the dequantized operands under
a derived elementwise bound, fp8_sdpa and a wrapped toy model at the reference's SQNR bars, and one graph capture."""
import pytest
import torch
import torch.nn.functional as F

import fp8_attention_ref as R
from ao_amd import ops
from ao_amd.prototype.attention import _fp8_sdpa_quantize, apply_low_precision_attention, fp8_sdpa

pytestmark = pytest.mark.gpu
DEV = "cuda"


def sqnr(ref, got):
    return (20 * torch.log10(ref.double().norm() / (ref.double() - got.double()).norm())).item()


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("groups", [1, 4])
@pytest.mark.parametrize("Sq,Skv", [(1, 1), (17, 65), (200, 129)])
@pytest.mark.parametrize("D", [64, 128])
def test_cast_bytes(D, Sq, Skv, groups, dtype, transposed):
    gen = torch.Generator().manual_seed(D + Sq + groups)
    B, Hkv = 2, 3
    q, k, v = (torch.randn(B, h, s, D, generator=gen).to(dtype) for h, s in ((Hkv * groups, Sq), (Hkv, Skv), (Hkv, Skv)))
    for t, g in ((q, groups), (k, 1), (v, 1)):
        t[0, 0:g] = 0                                        # kv head 0: all zeros, scale 1
        t[0, g:2 * g] = 0
        t[0, 2 * g - 1, -1, D // 2] = 2.0 ** -20              # kv head 1: a single 2^-20 (above 1e-12: the division)
        t[1, 0, 0, 3] = 448.0                                 # amax = 448 exactly: scale 1 by division
    want = R.cast_chain(q, k, v)
    # the transposed case: [B, S, H, D] memory seen as [B, H, S, D], the common caller; the kernel reads it in place
    on_gpu = [t.transpose(1, 2).contiguous().to(DEV).transpose(1, 2) if transposed else t.to(DEV) for t in (q, k, v)]
    got = _fp8_sdpa_quantize(*on_gpu)
    for w, g in zip(want[:3], got[:3]):
        assert g.is_contiguous() and torch.equal(g.cpu().view(torch.uint8), w.view(torch.uint8))
    for w, g in zip(want[3:], got[3:]):
        assert g.shape == (B, Hkv) and torch.equal(g.cpu().view(torch.int32), w.view(torch.int32))
    assert want[3][0, 0] == 1.0 and want[3][0, 1] == 2.0 ** -20 / 448.0


def check_kernel(D, Sq, Skv, causal, groups, spread=1.0, scale=None, out_dtype=torch.bfloat16):
    q8, k8, v8, dq, dk, dv = R.kernel_case(D, Sq, Skv, groups, spread)
    out = ops.fp8_attn_fwd(*(t.to(DEV) for t in (q8, k8, v8, dq, dk, dv)), is_causal=causal, scale=scale, out_dtype=out_dtype)
    assert out.dtype == out_dtype and out.shape == q8.shape
    v_deq = R.dequant(v8, dv).repeat_interleave(groups, 1)
    ref, p, l, logits = R.sdpa_f64(R.dequant(q8, dq, groups), R.dequant(k8, dk), R.dequant(v8, dv), causal, scale)
    err, bound = (out.cpu().double() - ref).abs(), R.kernel_bound(ref, p, l, v_deq, causal)
    print(f"max err / bound = {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    return logits


@pytest.mark.parametrize("groups", [1, 4])
@pytest.mark.parametrize("D,Sq,Skv,causal", R.KERNEL_SHAPES)
def test_kernel_against_float64(D, Sq, Skv, causal, groups):
    check_kernel(D, Sq, Skv, causal, groups)


def test_kernel_scale_spread_and_fp16():
    check_kernel(128, 65, 129, True, 4, scale=0.21, out_dtype=torch.float16)
    logits = check_kernel(64, 200, 200, False, 1, spread=8.0) * 1.4426950408889634
    assert (logits.amax(-1) - logits.amin(-1)).min() > 30  # the running maximum moves across KV tiles, the tail goes subnormal


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(2, 8, 256, 64), (1, 16, 256, 128)])
def test_fp8_sdpa_sqnr(shape, dtype, causal):
    gen = torch.Generator().manual_seed(shape[1])
    q, k, v = (torch.randn(shape, generator=gen).to(dtype) for _ in range(3))
    out = fp8_sdpa(q.to(DEV), k.to(DEV), v.to(DEV), is_causal=causal)
    assert out.dtype == dtype
    db = sqnr(R.sdpa_f64(q, k, v, causal)[0], out.cpu())
    print(f"SQNR {db:.2f} dB")
    assert db > 25.0


class Block(torch.nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads, self.qkv, self.proj = heads, torch.nn.Linear(dim, 3 * dim, bias=False), torch.nn.Linear(dim, dim, bias=False)

    def forward(self, x):
        B, S, E = x.shape
        q, k, v = (t.transpose(1, 2) for t in self.qkv(x).view(B, S, 3, self.heads, E // self.heads).unbind(2))
        return x + self.proj(F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B, S, E))


def test_wrapped_toy_model():
    torch.manual_seed(0)
    model = torch.nn.Sequential(Block(512, 8), Block(512, 8)).to(DEV, torch.bfloat16).eval()
    x = torch.randn(2, 128, 512, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        want = model(x)
        got = apply_low_precision_attention(model)(x)
    db = sqnr(want.cpu(), got.cpu())
    print(f"SQNR {db:.2f} dB")
    assert db > 20.0 and not torch.equal(want, got)


def test_graph_replay_gives_the_eager_bytes():
    gen = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(1, 4, 200, 128, generator=gen).to(torch.bfloat16).to(DEV) for _ in range(3))
    eager = fp8_sdpa(q, k, v, is_causal=True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fp8_sdpa(q, k, v, is_causal=True)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fp8_sdpa(q, k, v, is_causal=True)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
