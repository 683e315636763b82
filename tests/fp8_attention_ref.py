"""References for the FP8 attention tests: the cast chain in torch fp32 ops on the CPU, float64 SDPA on given operands with the parts the
kernel test's bound is built from, and a torch emulation of the kernel's own arithmetic (e4m3 cast of 256 p, fp32 sums)."""
import math

import torch

E4M3 = torch.float8_e4m3fn


def cast_chain(q, k, v):
    """triton_fp8_sdpa_quantize's arithmetic on CPU tensors [B, H, S, D]: (q8, k8, v8, dq, dk, dv)."""
    B, Hq, _, D = q.shape
    Hkv = k.shape[1]

    def one(x):
        xf = x.float().reshape(B, Hkv, -1)  # a kv head's rows; for q the group's query heads are adjacent
        amax = xf.abs().amax(dim=2)
        live = amax > 1e-12
        top = torch.full_like(amax, 448.0)  # tensor / tensor: an IEEE division (scalar / tensor is torch's reciprocal-then-multiply)
        scale = torch.where(live, top / amax, torch.ones_like(amax))
        descale = torch.where(live, amax / top, torch.ones_like(amax))
        codes = (xf * scale[:, :, None]).clamp(-448.0, 448.0).to(E4M3).reshape(x.shape)
        return codes, descale

    (q8, dq), (k8, dk), (v8, dv) = one(q), one(k), one(v)
    return q8, k8, v8, dq, dk, dv


def _visible(Sq, Skv, causal):
    i, j = torch.arange(Sq)[:, None], torch.arange(Skv)[None, :]
    return (j <= i) if causal else torch.ones(Sq, Skv, dtype=torch.bool)


def sdpa_f64(q, k, v, causal=False, scale=None):
    """float64 SDPA of q [B, Hq, Sq, D] against k, v [B, Hkv, Skv, D] (any float dtype): (out, p, l, logits) with p the softmax numerators
    against the row maximum (0 where masked), l their sums and logits the scaled scores (-inf where masked)."""
    groups = q.shape[1] // k.shape[1]
    q, k, v = q.double(), k.double().repeat_interleave(groups, 1), v.double().repeat_interleave(groups, 1)
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    logits = (q @ k.transpose(-1, -2)) * scale
    logits = logits.masked_fill(~_visible(q.shape[2], k.shape[2], causal), float("-inf"))
    p = torch.exp(logits - logits.amax(dim=-1, keepdim=True))
    l = p.sum(dim=-1, keepdim=True)
    return (p @ v) / l, p, l, logits


def dequant(codes, descale, groups=1):
    """code * descale in float64; descale [B, Hkv] of kv head h // groups."""
    return codes.double() * descale.double().repeat_interleave(groups, 1)[:, :, None, None]


def kernel_bound(ref, p, l, v_deq, causal):
    """The elementwise bound of the kernel test: half an e4m3 ulp on every normal 256 p, half a subnormal step after the 2^-8, the output
    rounding, fp32 accumulation slack.  v_deq: the dequantized V [B, Hq, Skv, D] (kv heads repeated)."""
    vabs = v_deq.abs()
    vis = _visible(p.shape[2], p.shape[3], causal).double()
    return (2.0 ** -4 * (p @ vabs) + 2.0 ** -18 * (vis @ vabs)) / l + 2.0 ** -8 * ref.abs() + 2.0 ** -16 * vabs.max()


def emulate_kernel(q8, k8, v8, dq, dk, dv, causal, scale, out_dtype):
    """The kernel's chain in torch fp32 on the CPU: base-2 logits under one folded multiplier, p against the row maximum, the row sum from
    the fp32 p, P cast as e4m3(256 p), fp32 products, dv * 2^-8 / l, one rounding to out_dtype."""
    groups = q8.shape[1] // k8.shape[1]
    rep = lambda t: t.repeat_interleave(groups, 1)
    scale = 1.0 / math.sqrt(q8.shape[-1]) if scale is None else scale
    c = (torch.tensor(scale * 1.4426950408889634, dtype=torch.float32) * rep(dq) * rep(dk))[:, :, None, None]
    t = (q8.float() @ rep(k8).float().transpose(-1, -2)) * c
    t = t.masked_fill(~_visible(q8.shape[2], k8.shape[2], causal), float("-inf"))
    p = torch.exp2(t - t.amax(dim=-1, keepdim=True))
    l = p.sum(dim=-1, keepdim=True)
    acc = (p * 256.0).to(E4M3).float() @ rep(v8).float()
    return (acc * (rep(dv)[:, :, None, None] / (l * 256.0))).to(out_dtype)


# (D, Sq, Skv, causal) of the kernel test: every tile edge of the 128-row query tile and the 64-row KV tile, a single row, a single key
KERNEL_SHAPES = [(D, sq, skv, False) for D in (64, 128) for sq, skv in ((1, 1), (1, 200), (64, 64), (65, 129), (129, 65), (200, 200))]
KERNEL_SHAPES += [(D, sq, skv, True) for D in (64, 128) for sq, skv in ((64, 64), (200, 200), (65, 129))]


def kernel_case(D, Sq, Skv, groups, spread=1.0, seed=0):
    """Codes and descales built on the CPU: B = 2, Hkv = 2, distinct descales per (batch, kv head) so that a wrong head index shows.
    `spread` scales the Q descales (8: the base-2 logits of every row spread over more than 30)."""
    gen = torch.Generator().manual_seed(seed + 131 * D + 17 * Sq + Skv + groups)
    B, Hkv = 2, 2
    q8 = torch.randn(B, Hkv * groups, Sq, D, generator=gen).to(E4M3)
    k8 = torch.randn(B, Hkv, Skv, D, generator=gen).to(E4M3)
    v8 = (2.0 * torch.randn(B, Hkv, Skv, D, generator=gen)).to(E4M3)
    steps = torch.arange(B * Hkv, dtype=torch.float32).reshape(B, Hkv)
    return q8, k8, v8, spread * (0.75 + 0.125 * steps), 1.5 - 0.25 * steps, 0.5 + 0.375 * steps
