#!/usr/bin/env python3
"""The low-bit optimizer step in one process: ops.optim_adam_step, one launch a parameter, as an HBM stream next to
torch.optim.AdamW(fused=True) on the same parameter and next to the same step written as a chain of eager PyTorch ops (what the reference
runs without its torch.compile step), and one step over a whole model's linears.

  cells  bf16 parameters of the Llama-3-8B shapes [4096, 4096], [14336, 4096] and [128256, 4096]; formats q8 (block 256), q4 (block 128), fp8
         (block 256) and plain (bf16 moments); AdamW, weight decay 1e-2, no amsgrad.  Every timed call takes the next of enough buffer
         sets (parameter, gradient, moments) that together they are at least 3 x the 256 MB last-level cache -- one set where a single set
         is already larger -- so no call finds its operands there.  Per cell:
           fused_us, fused_tbps      one launch; the algorithmic bytes over the time: q8 / fp8 10 B an element (p read and written, grad read,
                                     two codes read and written), q4 8 B, plain 14 B
           torch_fused_us            torch.optim.AdamW(fused=True).step() on a parameter of the same shape (bf16 moments: 14 B an element);
                                     no bar is set for this comparison
           eager_us                  the chain in eager torch ops on the same fields (dequantize by table lookup, the Adam arithmetic in fp32,
                                     block amax, the branch-free table descent, pack); speedup_vs_eager = eager_us / fused_us
  model  one AdamW8bit / AdamW4bit / AdamWFp8 / _AdamW step over the five Llama-3-8B linear shapes x 32 layers (160 parameters, 6.98 G elements;
         the gradients of one shape share one tensor), next to torch.optim.AdamW(fused=True) over the same parameters: step time (host clock
         around a step that ends in a synchronise, so the per-parameter launch overhead counts), and the sum of the per-shape cell times.
Device events around a window of calls, the median window of the replays, per call.
    python tools/bench_optim.py [--replays 5] [--only cells|model] [--shape RxC] [--format q8] [--fused-only] [--out profiles/optim.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ao_amd import ops  # noqa: E402
from ao_amd import optim as O  # noqa: E402
from ao_amd.optim import quant_utils as Q  # noqa: E402

SHAPES = [(4096, 4096), (14336, 4096), (128256, 4096)]
MODEL = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate", 14336, 4096), ("up", 14336, 4096), ("down", 4096, 14336)]
LAYERS = 32
LLC_BYTES = 256 << 20
FORMATS = {"q8": (Q.Q8_SIGNED, 256, 10), "q4": (Q.Q4_SIGNED, 128, 8), "fp8": (Q.FP8, 256, 10), "plain": (Q.PLAIN, 0, 14)}
BETAS, LR, WD, EPS = (0.9, 0.999), 1e-3, 1e-2, 1e-8


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


class Fields:
    """One buffer set: p, grad and the two moments in the flat form ops.optim_adam_step takes"""

    def __init__(self, fmt, n, dev):
        code, bs, _ = FORMATS[fmt]
        self.fmt, self.code, self.bs, self.n = fmt, code, bs, n
        self.p = torch.randn(n, device=dev, dtype=torch.bfloat16) * 0.05
        self.g = torch.randn(n, device=dev, dtype=torch.bfloat16) * 0.01
        if fmt == "plain":
            self.m = [torch.zeros(n, device=dev, dtype=torch.bfloat16), None, None]
            self.v = [torch.zeros(n, device=dev, dtype=torch.bfloat16), None, None]
        else:
            bits = {"q8": 8, "q4": 4}.get(fmt)
            codes = lambda: torch.zeros(n // 2 if fmt == "q4" else n, device=dev, dtype=torch.float8_e4m3fn if fmt == "fp8" else torch.uint8)  # noqa: E731
            scale = lambda: torch.zeros(n // bs, device=dev)  # noqa: E731
            self.m = [codes(), scale(), Q.make_qmap(bits, True, dev) if bits else None]
            self.v = [codes(), scale(), Q.make_qmap(bits, False, dev) if bits else None]

    def fused(self, scalars):
        ops.optim_adam_step(self.p, self.g, *self.m, *self.v, None, None, None, self.code, self.bs, scalars, True)

    # ---- the same step as a chain of eager torch ops (the project's own text of the contract; nothing here calls a kernel of ao_amd) ----
    def _dequant(self, s):
        codes, scale, qmap = s
        if self.fmt == "plain":
            return codes.float()
        if self.fmt == "fp8":
            v = codes.float()
        elif self.fmt == "q4":
            v = qmap[torch.stack([codes >> 4, codes & 15], dim=-1).view(-1).int()]
        else:
            v = qmap[codes.int()]
        return (v.view(-1, self.bs) * scale.view(-1, 1)).view(-1)

    def _quant(self, s, x):
        codes, scale, qmap = s
        if self.fmt == "plain":
            codes.copy_(x)
            return
        xb = x.view(-1, self.bs)
        sc = xb.abs().amax(-1).clip(1e-12)
        if self.fmt == "fp8":
            sc = sc / 448.0
            codes.copy_((xb / sc.view(-1, 1)).to(torch.float8_e4m3fn).view(-1))
            scale.copy_(sc)
            return
        y = (xb / sc.view(-1, 1)).view(-1)
        top = qmap.numel()
        c = torch.where(y >= qmap[top // 2], top // 2, 0)
        step = top // 4
        while step >= 1:
            c += torch.where(y >= qmap[c + step], step, 0)
            step //= 2
        up = (c + 1).clip(max=top - 1)
        lo_v, up_v = qmap[c], qmap[up]
        c = torch.where(y - lo_v >= (up_v - lo_v) * 0.5, up, c).to(torch.uint8)
        codes.copy_((c[::2] << 4) | c[1::2] if self.fmt == "q4" else c)
        scale.copy_(sc)

    def eager(self, lr, step):
        p32, g32 = self.p.float(), self.g.float()
        p32 = p32 - lr * WD * p32
        bc1, bc2 = 1 - BETAS[0] ** step, 1 - BETAS[1] ** step
        m = self._dequant(self.m).lerp(g32, 1 - BETAS[0])
        v = self._dequant(self.v).lerp(g32.square(), 1 - BETAS[1])
        self._quant(self.m, m)
        self._quant(self.v, v)
        denom = (v.sqrt() / bc2.sqrt()) + EPS
        self.p.copy_(p32 - lr * (m / bc1) / denom)

    def bytes(self):
        return sum(t.numel() * t.element_size() for t in [self.p, self.g, self.m[0], self.v[0]])


def cell(r, c, fmt, dev, replays, fused_only=False, calls=None):
    n = r * c
    probe = Fields(fmt, 4096, dev)
    per_set = probe.bytes() * (n // 4096)
    nbuf = max(1, -(-3 * LLC_BYTES // per_set))
    sets = [Fields(fmt, n, dev) for _ in range(nbuf)]
    scalars = O.step_scalars(torch.tensor(LR), BETAS[0], BETAS[1], WD, EPS, torch.tensor(5.0))
    calls = calls or nbuf * -(-48 // nbuf)
    rec = {"kind": "cell", "format": fmt, "R": r, "C": c, "block_size": FORMATS[fmt][1], "buffers": nbuf, "calls": calls, "replays": replays,
           "bytes_per_element": FORMATS[fmt][2], "grid": ops.optim_grid(n)}
    rec["fused_us"] = window_us(lambda i: sets[i % nbuf].fused(scalars), calls, replays)
    rec["fused_tbps"] = n * FORMATS[fmt][2] / (rec["fused_us"] * 1e-6) / 1e12
    if fused_only:
        return rec
    params = [torch.nn.Parameter(s.p.clone()) for s in sets]
    for q, s in zip(params, sets):
        q.grad = s.g
    opts = [torch.optim.AdamW([q], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, fused=True) for q in params]
    rec["torch_fused_us"] = window_us(lambda i: opts[i % nbuf].step(), calls, replays)
    rec["torch_fused_tbps"] = n * 14 / (rec["torch_fused_us"] * 1e-6) / 1e12
    del opts, params
    torch.cuda.empty_cache()
    lr, step = torch.tensor(LR), torch.tensor(5.0)
    eager_calls = max(nbuf, 4)
    with torch.no_grad():
        rec["eager_us"] = window_us(lambda i: sets[i % nbuf].eager(lr, step), eager_calls, replays)
    rec["eager_calls"] = eager_calls
    rec["speedup_vs_eager"] = rec["eager_us"] / rec["fused_us"]
    rec["fused_over_torch_fused"] = rec["fused_us"] / rec["torch_fused_us"]
    return rec


def model(name, make_opt, dev, replays):
    grads = {(n, k): torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.01 for _, n, k in MODEL}
    params = []
    for _ in range(LAYERS):
        for _, n, k in MODEL:
            q = torch.nn.Parameter(torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.05)
            q.grad = grads[(n, k)]
            params.append(q)
    opt = make_opt(params)
    for _ in range(2):
        opt.step()
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        t0 = time.perf_counter()
        opt.step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    elements = sum(q.numel() for q in params)
    return {"kind": "model", "optimizer": name, "parameters": len(params), "elements": elements, "replays": replays,
            "step_ms": statistics.median(times), "step_ms_min": min(times), "step_ms_max": max(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5, help="timed windows per figure (the median is recorded; at least 5)")
    ap.add_argument("--only", choices=["cells", "model"], default=None)
    ap.add_argument("--shape", default=None, help="one shape RxC instead of the three")
    ap.add_argument("--format", default=None, choices=list(FORMATS))
    ap.add_argument("--fused-only", action="store_true", help="only the fused launch (for a profiler run of one cell)")
    ap.add_argument("--calls", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.replays < 5 and not args.fused_only:
        ap.error("--replays must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_optim.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    shapes = [tuple(int(v) for v in args.shape.split("x"))] if args.shape else SHAPES
    formats = [args.format] if args.format else list(FORMATS)
    if args.only != "model":
        for r, c in shapes:
            for fmt in formats:
                emit(cell(r, c, fmt, dev, args.replays, args.fused_only, args.calls))
                torch.cuda.empty_cache()
    if args.only != "cells" and not args.fused_only:
        for name, make in (("AdamW8bit", lambda p: O.AdamW8bit(p, lr=LR)), ("AdamW4bit", lambda p: O.AdamW4bit(p, lr=LR)),
                           ("AdamWFp8", lambda p: O.AdamWFp8(p, lr=LR)), ("_AdamW", lambda p: O._AdamW(p, lr=LR)),
                           ("torch.optim.AdamW(fused=True)", lambda p: torch.optim.AdamW(p, lr=LR, fused=True))):
            if args.format and not name.lower().endswith({"q8": "8bit", "q4": "4bit", "fp8": "fp8", "plain": "_adamw"}[args.format]):
                continue
            emit(model(name, make, dev, args.replays))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
