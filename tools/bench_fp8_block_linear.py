#!/usr/bin/env python3
"""The blockwise float8 linears measured (1 x 128 activation blocks, 128 x 128 weight blocks):
  * decode: one token (bs = 1) through the Llama-3-8B five-shape x 32-layer linears and through four DeepSeek-V3 dense shapes, cold
    weights (every layer its own weights, far beyond the caches), hipGraph replay, tok/s and the weight bytes per second as a fraction
    of 8 TB/s -- for the blockwise linear (by the host rule, and with the cast forced into the GEMM), the rowwise fp8 dynamic linear
    (the yardstick: the same weight bytes; per 128 weight rows the blockwise weight carries K/128 scales where the rowwise one carries
    128) and PyTorch's bf16 F.linear, all in this one process;
  * --fused: M = 1 .. 16, the cast fused into the GEMM against two launches, weights rotated through copies so that they come from HBM:
    what ops.FP8_BLOCK_FUSED_MAX_ROWS should be;
  * --sweep: M = 16 .. 256 with each form forced (ao_fp8_block_linear_set_form): what AO_FP8_BLOCK_STREAM_MAX_ROWS should be.
  * --fit FILE: the hand-off row count and the fused rule a results file gives (no GPU).
    python tools/bench_fp8_block_linear.py [--steps 20] [--fused] [--sweep] [--tag LABEL] [--out profiles/fp8_block_linear.jsonl]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ao_amd import ops  # noqa: E402

HBM_BPS = 8.0e12  # MI355X HBM3E peak
FUSED_M = tuple(range(1, 17))
SWEEP_M = (16, 17, 24, 32, 33, 48, 64, 65, 96, 128, 192, 256)
COLD_BYTES = 512 << 20  # rotate a sweep's weight through copies worth this much: twice the last-level cache
# (name, N, K): DeepSeek-V3's dense projections -- four 7168 x 2048, 7168 x 18432, 18432 x 7168, 1536 x 7168 -- one "layer" of this list
DEEPSEEK_V3_DENSE = [("proj_a", 7168, 2048), ("proj_b", 7168, 2048), ("proj_c", 7168, 2048), ("proj_d", 7168, 2048),
                     ("down", 7168, 18432), ("up", 18432, 7168), ("q_a", 1536, 7168)]


def quantize(w, kind):
    if kind == "block":
        return ops.fp8_quantize_block_128x128(w)
    return ops.fp8_quantize_rowwise(w)


FAMILIES = {
    # name: (weight kind, call)
    "block_fp8": ("block", lambda x, q, s: ops.fp8_block_linear(x, q, s)),  # the host rule: ops.FP8_BLOCK_FUSED_MAX_ROWS
    "block_fp8_fused": ("block", lambda x, q, s: ops.fp8_block_linear(x, q, s, fuse=True)),
    "dyn_fp8": ("row", lambda x, q, s: ops.fp8_linear(x, q, s)),
    "bf16": ("bf16", lambda x, w, s: F.linear(x, w)),
}


class Linears:
    def __init__(self, dev, layers, shapes, family):
        kind, self.call = FAMILIES[family]
        self.weights = []
        g = torch.Generator(device=dev).manual_seed(0)
        for _ in range(layers):
            for name, n, k in shapes:
                w = torch.randn(n, k, device=dev, dtype=torch.bfloat16, generator=g) * 0.02
                self.weights.append((w, None) if kind == "bf16" else quantize(w, kind))
                del w
        self.x = {}
        self.bytes = sum(q.numel() * q.element_size() + (0 if s is None else s.numel() * 4) for q, s in self.weights)

    def step(self, batch):
        for q, s in self.weights:
            k = q.shape[1]
            if (batch, k) not in self.x:
                self.x[(batch, k)] = torch.randn(batch, k, device=q.device, dtype=torch.bfloat16)
            self.call(self.x[(batch, k)], q, s)


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


def decode(args, dev, shapes, layers):
    stream = torch.cuda.Stream(device=dev)
    res = {}
    with torch.no_grad():
        for family in FAMILIES:
            m = Linears(dev, layers, shapes, family)
            sec = graph_time(lambda: m.step(1), stream, args.steps, args.warmup)
            res[family] = {"tok_s": 1.0 / sec, "step_us": sec * 1e6, "weight_bytes": m.bytes, "hbm_fraction": m.bytes / sec / HBM_BPS}
            del m
            torch.cuda.empty_cache()
    res["block_fp8"]["vs_bf16"] = res["block_fp8"]["tok_s"] / res["bf16"]["tok_s"]
    res["block_fp8"]["vs_dyn"] = res["block_fp8"]["tok_s"] / res["dyn_fp8"]["tok_s"]
    res["block_fp8_fused"]["vs_dyn"] = res["block_fp8_fused"]["tok_s"] / res["dyn_fp8"]["tok_s"]
    res["layers"] = layers
    res["fused_max_rows"] = ops.FP8_BLOCK_FUSED_MAX_ROWS
    res["route_bs1"] = {name: ops.fp8_block_linear_route(1, n, k) for name, n, k in shapes}
    return res


def time_us(fn, copies, reps):
    for i in range(copies):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i % copies)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _cold_weights(dev, n, k):
    copies = max(2, -(-COLD_BYTES // (n * k)))
    ws = []
    for _ in range(copies):
        w = torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.02
        ws.append(quantize(w, "block"))
        del w
    return copies, ws


TAG = None


def emit(r, out):
    if TAG:
        r = {"tag": TAG, **r}
    print(json.dumps(r), flush=True)
    if out:
        out.write(json.dumps(r) + "\n")
        out.flush()


def fused(args, dev, out):
    for name, n, k in bench.LLAMA3_8B_UNMERGED:
        copies, ws = _cold_weights(dev, n, k)
        reps = max(args.reps, 2 * copies)
        for m in FUSED_M:
            x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
            r = {"fused": name, "M": m, "N": n, "K": k, "copies": copies, "reps": reps}
            r["fused_us"] = time_us(lambda i: ops.fp8_block_linear(x, *ws[i], fuse=True), copies, reps)
            r["two_launch_us"] = time_us(lambda i: ops.fp8_block_linear(x, *ws[i], fuse=False), copies, reps)
            emit(r, out)
        del ws
        torch.cuda.empty_cache()


def sweep(args, dev, out):
    for name, n, k in bench.LLAMA3_8B_UNMERGED:
        copies, ws = _cold_weights(dev, n, k)
        reps = max(args.reps, 2 * copies)
        for m in SWEEP_M:
            x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
            aq, a_s = ops.fp8_quantize_block_1x128(x)
            r = {"sweep": name, "M": m, "N": n, "K": k, "copies": copies, "reps": reps, "route": ops.fp8_block_linear_kernel_name(m, n, k)}
            for form, fname in ((1, "stream"), (2, "tile")):
                ops.fp8_block_linear_set_form(form)
                try:
                    r[f"{fname}_us"] = time_us(lambda i: ops.fp8_block_mm(aq, a_s, *ws[i]), copies, reps)
                finally:
                    ops.fp8_block_linear_set_form(0)
            emit(r, out)
        del ws
        torch.cuda.empty_cache()


def fit(path):
    """From a results file: the seam s (stream up to s rows, tiled beyond) with the least GEMM time summed over the five shapes and every
    swept M, and the largest M up to which the fused launch is not slower than two, summed over the shapes."""
    rows = [json.loads(l) for l in open(path) if l.strip()]
    sw = [r for r in rows if "sweep" in r]
    if sw:
        ms = sorted({r["M"] for r in sw})
        total = {seam: sum(r["stream_us"] if r["M"] <= seam else r["tile_us"] for r in sw) for seam in [0] + ms}
        print(json.dumps({"fit": "seam", "seam": min(total, key=total.get), "summed_us_by_seam": {str(k): round(v, 1) for k, v in total.items()}}))
    fu = [r for r in rows if "fused" in r]
    if fu:
        by_m = {m: (sum(r["fused_us"] for r in fu if r["M"] == m), sum(r["two_launch_us"] for r in fu if r["M"] == m)) for m in sorted({r["M"] for r in fu})}
        best = 0
        for m, (f, t) in by_m.items():
            if f > t:
                break
            best = m
        print(json.dumps({"fit": "fused_max_rows", "rows": best, "summed_us_fused_two": {str(m): [round(f, 1), round(t, 1)] for m, (f, t) in by_m.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=bench.N_LAYERS)
    ap.add_argument("--ds-layers", type=int, default=8, help="copies of the DeepSeek-V3 dense shape list (334 MB of codes each)")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default=None, help="a label written into every record of this run")
    ap.add_argument("--fit", default=None, metavar="JSONL", help="no GPU: print the fitted seam and fused rule of a results file")
    args = ap.parse_args()
    if args.fit:
        return fit(args.fit)
    global TAG
    TAG = args.tag
    if not torch.cuda.is_available():
        sys.exit("bench_fp8_block_linear.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None
    if not args.no_decode:
        emit({"decode_bs1_llama3_8b_five_shape": decode(args, dev, bench.LLAMA3_8B_UNMERGED, args.layers)}, out)
        emit({"decode_bs1_deepseek_v3_dense": decode(args, dev, DEEPSEEK_V3_DENSE, args.ds_layers)}, out)
    if args.fused:
        fused(args, dev, out)
    if args.sweep:
        sweep(args, dev, out)


if __name__ == "__main__":
    main()
