#!/usr/bin/env python3
"""The int8 / float8 weight-only linears measured:
  * decode: one token (bs = 1) through the Llama-3-8B five-shape x 32-layer linears, cold weights (bench.py's model: every layer its own
    weights, far beyond the caches), hipGraph replay, tok/s and the weight bytes per second as a fraction of 8 TB/s -- for the two
    weight-only linears, the int8 / fp8 dynamic-activation linears and PyTorch's bf16 F.linear, all in this one process;
  * --sweep: M = 1 .. 256 on the five shapes, us per linear with each form forced (ao_wo8_linear_set_form), the weights rotated through
    enough copies that they come from HBM: what the hand-off row count of wo8_route is fitted on.
  * --fit FILE: the hand-off row counts a sweep file gives (no GPU).
    python tools/bench_wo8_linear.py [--steps 20] [--sweep] [--out profiles/wo8_linear.jsonl]"""
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
SWEEP_M = (1, 2, 4, 8, 16, 17, 24, 32, 33, 48, 64, 65, 96, 128, 192, 256)
COLD_BYTES = 512 << 20  # rotate a sweep's weight through copies worth this much: twice the last-level cache


def quantize(w, kind):
    """(codes, scale) of a bf16 weight: per-row int8 or e4m3, the casts Int8Tensor / Float8Tensor.from_hp run."""
    return ops.int8_quantize_rowwise(w) if kind == "int8" else ops.fp8_quantize_rowwise(w)


FAMILIES = {
    # name: (weight kind, call)
    "wo_int8": ("int8", lambda x, q, s: ops.int8_wo_linear(x, q, s)),
    "wo_fp8": ("fp8", lambda x, q, s: ops.fp8_wo_linear(x, q, s)),
    "dyn_int8": ("int8", lambda x, q, s: ops.int8_linear(x, q, s)),
    "dyn_fp8": ("fp8", lambda x, q, s: ops.fp8_linear(x, q, s)),
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


def decode(args, dev):
    stream = torch.cuda.Stream(device=dev)
    res = {}
    with torch.no_grad():
        for family in FAMILIES:
            m = Linears(dev, args.layers, bench.LLAMA3_8B_UNMERGED, family)
            sec = graph_time(lambda: m.step(1), stream, args.steps, args.warmup)
            res[family] = {"tok_s": 1.0 / sec, "step_us": sec * 1e6, "weight_bytes": m.bytes, "hbm_fraction": m.bytes / sec / HBM_BPS}
            del m
            torch.cuda.empty_cache()
    for family in ("wo_int8", "wo_fp8"):
        res[family]["vs_bf16"] = res[family]["tok_s"] / res["bf16"]["tok_s"]
        res[family]["vs_dyn"] = res[family]["tok_s"] / res["dyn_" + family[3:]]["tok_s"]
    res["route_bs1"] = {name: ops.wo8_route(ops.WO8_FMT_INT8, 1, n, k) for name, n, k in bench.LLAMA3_8B_UNMERGED}
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


def sweep(args, dev, out):
    for name, n, k in bench.LLAMA3_8B_UNMERGED:
        copies = max(2, -(-COLD_BYTES // (n * k)))
        ws = {"int8": [], "fp8": []}
        for _ in range(copies):
            w = torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.02
            for kind in ws:
                ws[kind].append(quantize(w, kind))
            del w
        reps = max(args.reps, 2 * copies)
        for m in SWEEP_M:
            x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
            r = {"sweep": name, "M": m, "N": n, "K": k, "copies": copies, "reps": reps}
            for kind, fmt, op in (("int8", ops.WO8_FMT_INT8, ops.int8_wo_linear), ("fp8", ops.WO8_FMT_E4M3, ops.fp8_wo_linear)):
                r[f"{kind}_route"] = ops.wo8_route(fmt, m, n, k)["kernel"]
                for form, fname in ((1, "stream"), (2, "tile")):
                    ops.wo8_set_form(form)
                    try:
                        r[f"{kind}_{fname}_us"] = time_us(lambda i: op(x, *ws[kind][i]), copies, reps)
                    finally:
                        ops.wo8_set_form(0)
            print(json.dumps(r), flush=True)
            if out:
                out.write(json.dumps(r) + "\n")
                out.flush()
        del ws
        torch.cuda.empty_cache()


def fit(path):
    """The hand-off row count per format from a sweep file: the seam s (stream up to s rows, tiled beyond) with the least time summed over
    the five shapes and every swept M; per candidate the sum, so that the margin shows."""
    rows = [r for r in (json.loads(l) for l in open(path) if l.strip()) if "sweep" in r]
    ms = sorted({r["M"] for r in rows})
    for kind in ("int8", "fp8"):
        total = {}
        for seam in [0] + ms:
            total[seam] = sum(r[f"{kind}_stream_us"] if r["M"] <= seam else r[f"{kind}_tile_us"] for r in rows)
        best = min(total, key=total.get)
        print(json.dumps({"fit": kind, "seam": best, "summed_us_by_seam": {str(k): round(v, 1) for k, v in total.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=bench.N_LAYERS)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fit", default=None, metavar="JSONL", help="no GPU: print the fitted hand-off row counts of a sweep file")
    args = ap.parse_args()
    if args.fit:
        return fit(args.fit)
    if not torch.cuda.is_available():
        sys.exit("bench_wo8_linear.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None
    if not args.no_decode:
        r = {"decode_bs1_llama3_8b_five_shape": decode(args, dev)}
        print(json.dumps(r), flush=True)
        if out:
            out.write(json.dumps(r) + "\n")
            out.flush()
    if args.sweep:
        sweep(args, dev, out)


if __name__ == "__main__":
    main()
