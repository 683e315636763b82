#!/usr/bin/env python3
"""The MX dense linears measured:
  * decode: one token (bs = 1) through the Llama-3-8B five-shape x 32-layer linears, cold weights (bench.py's model: every layer its own
    weights, far beyond the caches), hipGraph replay, tok/s for MXFP4, MXFP8 and the product's int4 path in the same process;
  * --sweep: M = 1 .. 16384 on the five shapes, us per linear for MXFP4 / MXFP8 (the product route and both forms forced), bf16 torch.mm
    and the fp8 rowwise dynamic linear.
    python tools/bench_mx_linear.py [--steps 20] [--sweep] [--out profiles/mx_linear.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ao_amd import ops  # noqa: E402

HBM_BPS = 8.0e12  # MI355X HBM3E peak


class MxLinears:
    def __init__(self, dev, layers, shapes, fmt):
        self.fmt, self.weights = fmt, []
        g = torch.Generator(device=dev).manual_seed(0)
        for _ in range(layers):
            for name, n, k in shapes:
                w = torch.randn(n, k, device=dev, dtype=torch.bfloat16, generator=g) * 0.02
                q, s = ops.mx_quantize(w, fmt, "rceil")
                del w
                self.weights.append((q.view(torch.uint8), s.view(torch.uint8), n, k))
        self.x = {}
        self.bytes = sum(q.numel() + s.numel() for q, s, _, _ in self.weights)

    def step(self, batch):
        for q, s, n, k in self.weights:
            if (batch, k) not in self.x:
                self.x[(batch, k)] = torch.randn(batch, k, device=q.device, dtype=torch.bfloat16)
            ops.mx_linear(self.x[(batch, k)], q, s, None, self.fmt, "rceil")


def graph_time(fn, stream, steps, warmup):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / steps


def decode(args, dev):
    stream = torch.cuda.Stream(device=dev)
    res = {}
    int4 = bench.Int4Linears(dev, bench.N_LAYERS, bench.LLAMA3_8B_UNMERGED)
    sec = graph_time(lambda: int4.step(1, torch.cuda.current_stream().cuda_stream), stream, args.steps, args.warmup)
    int4_bytes = sum(q.numel() * q.element_size() + s.numel() * s.element_size() for q, s, _, _, _ in int4.weights)
    res["int4"] = {"tok_s": 1.0 / sec, "step_us": sec * 1e6, "hbm_fraction": int4_bytes / sec / HBM_BPS}
    del int4
    torch.cuda.empty_cache()
    for fmt, tag in ((ops.MX_FMT_E2M1, "mxfp4"), (ops.MX_FMT_E4M3, "mxfp8")):
        m = MxLinears(dev, bench.N_LAYERS, bench.LLAMA3_8B_UNMERGED, fmt)
        sec = graph_time(lambda: m.step(1), stream, args.steps, args.warmup)
        res[tag] = {"tok_s": 1.0 / sec, "step_us": sec * 1e6, "hbm_fraction": m.bytes / sec / HBM_BPS,
                    "kernel": ops.mx_linear_kernel_name(fmt, 1, 4096, 4096)}
        del m
        torch.cuda.empty_cache()
    return res


def time_us(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def sweep(dev, out):
    from ao_amd.quantization import Float8DynamicActivationFloat8WeightConfig, PerRow, quantize_

    rows = []
    for name, n, k in bench.LLAMA3_8B_UNMERGED:
        w = torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.02
        ws = {fmt: [t.view(torch.uint8) for t in ops.mx_quantize(w, fmt, "rceil")] for fmt in (ops.MX_FMT_E2M1, ops.MX_FMT_E4M3)}
        lin = torch.nn.Linear(k, n, bias=False, dtype=torch.bfloat16, device=dev)
        with torch.no_grad():
            lin.weight.copy_(w)
        quantize_(lin, Float8DynamicActivationFloat8WeightConfig(granularity=PerRow()))
        for m in (1, 2, 4, 8, 16, 32, 48, 64, 96, 128, 256, 512, 1024, 2048, 4096, 8192, 16384):
            x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
            r = {"shape": name, "M": m, "N": n, "K": k}
            r["bf16_mm_us"] = time_us(lambda: torch.mm(x, w.t()))
            with torch.no_grad():
                r["fp8_rowwise_us"] = time_us(lambda: lin(x))
            for fmt, tag in ((ops.MX_FMT_E2M1, "mxfp4"), (ops.MX_FMT_E4M3, "mxfp8")):
                q, s = ws[fmt]
                r[f"{tag}_kernel"] = ops.mx_linear_kernel_name(fmt, m, n, k)
                r[f"{tag}_us"] = time_us(lambda: ops.mx_linear(x, q, s, None, fmt, "rceil"))
                for form, fname in ((1, "stream"), (2, "tile")):
                    if form == 1 and m > 256:
                        continue
                    ops.mx_linear_set_form(form)
                    try:
                        r[f"{tag}_{fname}_us"] = time_us(lambda: ops.mx_linear(x, q, s, None, fmt, "rceil", fuse=form == 1))
                    finally:
                        ops.mx_linear_set_form(0)
            rows.append(r)
            print(json.dumps(r), flush=True)
            if out:
                out.write(json.dumps(r) + "\n")
                out.flush()
        del w, ws, lin
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None
    if not args.no_decode:
        r = {"decode_bs1_llama3_8b_five_shape": decode(args, dev)}
        print(json.dumps(r), flush=True)
        if out:
            out.write(json.dumps(r) + "\n")
    if args.sweep:
        sweep(dev, out)


if __name__ == "__main__":
    main()
