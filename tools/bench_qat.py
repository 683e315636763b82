#!/usr/bin/env python3
"""Quantization-aware training in one process: the four fused fake-quantize launches as HBM streams next to the same
chains written in eager PyTorch ops, and forward + backward of FakeQuantizedLinear next to bf16 nn.Linear autograd and next to the same
module on the eager chains.

  kernels  the Llama-3-8B weight shapes [4096, 4096], [14336, 4096], [4096, 14336] and activations of 8192 rows x 4096 / 14336, bf16.
           Every timed call takes the next of enough input buffers that together they are 3 x the 256 MB last-level cache, so no call
           finds its input there; a window is whole turns through the buffers, at least 96 calls.  Per shape and quantizer (int4 at
           group sizes 32 and 128; fp8 rowwise):
             fwd_us / bwd_us             ops.qat_*_fake_quantize / _bwd, one launch each
             fwd_tbps / bwd_tbps         the algorithmic bytes over the time: 4 B an element forward (read 2, write 2), 6 B backward
                                         (read the input and the gradient, write the gradient)
             eager_fwd_us                the chain in eager ops under no_grad
             eager_fwd_bwd_us            the chain under autograd, forward and backward (its backward needs what its forward saved)
             speedup_fwd                 eager_fwd_us / fwd_us
             speedup_fwd_bwd             eager_fwd_bwd_us / (fwd_us + bwd_us)
  linears  the three weight shapes at M = 8192 tokens, bias-free, input and weight requiring grad; per config pair (int4 weight-only at
           group size 128; fp8 activation + fp8 weight): fused_fwd_bwd_us (FakeQuantizedLinear), eager_fwd_bwd_us (the same module on the
           eager chains), bf16_fwd_bwd_us (nn.Linear), overhead_vs_bf16 = fused / bf16, speedup_vs_eager = eager / fused.
Device events around a window of calls, the median window of the replays, per call.
    python tools/bench_qat.py [--replays 7] [--only kernels|linears] [--out profiles/qat.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ao_amd import ops  # noqa: E402
from ao_amd.quantization.qat import FakeQuantizedLinear, Float8FakeQuantizeConfig, Int4WeightFakeQuantizeConfig  # noqa: E402

WEIGHTS = [(4096, 4096), (14336, 4096), (4096, 14336)]
ACTIVATIONS = [(8192, 4096), (8192, 14336)]
M_TOKENS = 8192
LLC_BYTES = 256 << 20


def window_us(fn, calls, replays):
    """Median over `replays` windows of `calls` calls fn(i), per call; one untimed window first."""
    for i in range(calls):
        fn(i)
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / calls)
    return statistics.median(times)


class _StraightThrough(torch.autograd.Function):
    """y in the forward, the identity in the backward: round and the e4m3 cast of the eager chains"""

    @staticmethod
    def forward(ctx, x, kind):
        return torch.round(x) if kind == "round" else x.to(torch.float8_e4m3fn).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        return g, None


def eager_int4(w, g):
    x = w.to(torch.float32).view(w.shape[0], -1, g)
    hi, lo = torch.amax(x, dim=-1, keepdim=True), torch.amin(x, dim=-1, keepdim=True)
    s = torch.clamp(hi - lo, min=1e-6) / 15
    z = lo + s * 8
    q = _StraightThrough.apply((x - lo) / s, "round").clamp(0, 15) - 8
    return (q * s + z).view(w.shape).to(w.dtype)


def eager_fp8(x, lb=None, ub=None):
    a = x.abs().amax(dim=-1, keepdim=True)
    if lb is not None or ub is not None:
        a = torch.clamp(a, min=lb, max=ub)
    s = (a / 448.0).to(torch.float32)
    q = _StraightThrough.apply((x.to(torch.float32) / s).clamp(-448.0, 448.0), "e4m3")
    return (q * s).to(x.dtype)


class EagerFakeQuantizedLinear(torch.nn.Linear):
    def forward(self, x):
        if self.act is not None:
            x = self.act(x)
        return F.linear(x, self.wq(self.weight), self.bias)


def kernels(r, c, what, dev, replays):
    nbuf = max(2, -(-3 * LLC_BYTES // (r * c * 2)))
    xs = [torch.randn(r, c, device=dev, dtype=torch.bfloat16) * (0.02 if what == "weight" else 1.0) for _ in range(nbuf)]
    gs = [torch.randn(r, c, device=dev, dtype=torch.bfloat16) * 1e-3 for _ in range(nbuf)]
    forms = {"fp8": (lambda x: ops.qat_fp8_fake_quantize_rowwise(x), lambda x, g: ops.qat_fp8_fake_quantize_rowwise_bwd(x, g), eager_fp8)}
    if what == "weight":
        for gsz in (32, 128):
            forms[f"int4_g{gsz}"] = (lambda x, gsz=gsz: ops.qat_int4_fake_quantize(x, gsz),
                                     lambda x, g, gsz=gsz: ops.qat_int4_fake_quantize_bwd(x, g, gsz), lambda x, gsz=gsz: eager_int4(x, gsz))
    calls = nbuf * -(-96 // nbuf)  # whole turns through the buffers, at least 96 calls a window
    recs = []
    for name, (fwd, bwd, eager) in forms.items():
        rec = {"kind": "kernel", "quantizer": name, "operand": what, "R": r, "C": c, "buffers": nbuf, "calls": calls, "replays": replays}
        rec["fwd_us"] = window_us(lambda i: fwd(xs[i % nbuf]), calls, replays)
        rec["bwd_us"] = window_us(lambda i: bwd(xs[i % nbuf], gs[i % nbuf]), calls, replays)
        rec["fwd_tbps"] = r * c * 4 / (rec["fwd_us"] * 1e-6) / 1e12
        rec["bwd_tbps"] = r * c * 6 / (rec["bwd_us"] * 1e-6) / 1e12
        with torch.no_grad():
            rec["eager_fwd_us"] = window_us(lambda i: eager(xs[i % nbuf]), calls, replays)

        def eager_step(i):
            x = xs[i % nbuf].detach().requires_grad_(True)
            eager(x).backward(gs[i % nbuf])

        rec["eager_fwd_bwd_us"] = window_us(eager_step, calls, replays)
        rec["speedup_fwd"] = rec["eager_fwd_us"] / rec["fwd_us"]
        rec["speedup_fwd_bwd"] = rec["eager_fwd_bwd_us"] / (rec["fwd_us"] + rec["bwd_us"])
        recs.append(rec)
    return recs


def linear(n, k, dev, replays):
    m = M_TOKENS
    x = torch.randn(m, k, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    go = torch.randn(m, n, device=dev, dtype=torch.bfloat16) * 0.01
    ref = torch.nn.Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16)

    def step(mod):
        x.grad = mod.weight.grad = None
        mod(x).backward(go)

    bf16_us = window_us(lambda i: step(ref), 8, replays)
    pairs = {
        "int4_g128": (None, Int4WeightFakeQuantizeConfig(group_size=128), None, lambda w: eager_int4(w, 128)),
        "fp8": (Float8FakeQuantizeConfig(), Float8FakeQuantizeConfig(), eager_fp8, eager_fp8),
    }
    recs = []
    for name, (act, wc, eager_act, eager_w) in pairs.items():
        fused = FakeQuantizedLinear.from_linear(ref, act, wc)
        eager = EagerFakeQuantizedLinear(k, n, bias=False, device=dev, dtype=torch.bfloat16)
        eager.weight, eager.act, eager.wq = ref.weight, eager_act, eager_w
        rec = {"kind": "linear", "pair": name, "M": m, "N": n, "K": k, "replays": replays, "bf16_fwd_bwd_us": bf16_us}
        rec["fused_fwd_bwd_us"] = window_us(lambda i: step(fused), 8, replays)
        rec["eager_fwd_bwd_us"] = window_us(lambda i: step(eager), 8, replays)
        rec["overhead_vs_bf16"] = rec["fused_fwd_bwd_us"] / bf16_us
        rec["speedup_vs_eager"] = rec["eager_fwd_bwd_us"] / rec["fused_fwd_bwd_us"]
        recs.append(rec)
    x.grad = ref.weight.grad = None
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=7, help="timed windows per figure (the median is recorded; at least 5)")
    ap.add_argument("--only", choices=["kernels", "linears"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.replays < 5:
        ap.error("--replays must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_qat.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None
    jobs = []
    if args.only != "linears":
        jobs += [lambda r=r, c=c: kernels(r, c, "weight", dev, args.replays) for r, c in WEIGHTS]
        jobs += [lambda r=r, c=c: kernels(r, c, "activation", dev, args.replays) for r, c in ACTIVATIONS]
    if args.only != "kernels":
        jobs += [lambda n=n, k=k: linear(n, k, dev, args.replays) for n, k in WEIGHTS]
    for job in jobs:
        for rec in job():
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
