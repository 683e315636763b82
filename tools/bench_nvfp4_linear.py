#!/usr/bin/env python3
"""The NVFP4 linears measured:
  * decode: one token (bs = 1) through the Llama-3-8B five-shape x 32-layer linears, cold weights (bench.py's model: every layer its own
    weights, far beyond the caches), hipGraph replay, tok/s and the weight bytes per second as a fraction of 8 TB/s -- for the NVFP4
    weight-only linear, the NVFP4 dynamic linear (per-tensor amax + cast + GEMM), int4 (tinygemm layout, group 128), MXFP4 and PyTorch's
    bf16 F.linear, all in this one process.  NVFP4 reads 0.5625 bytes a weight: half a byte of codes and one scale byte per 16;
  * --sweep: M = 1 .. 256 on the five shapes, us per linear with each form forced (ao_nvfp4_linear_set_form), the weights rotated
    through enough copies that they come from HBM: what the hand-off row counts of nvfp4_route are fitted on.
  * --fit FILE: the hand-off row counts a sweep file gives (no GPU).
    python tools/bench_nvfp4_linear.py [--steps 20] [--sweep] [--out profiles/nvfp4_linear.jsonl]"""
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


def nvfp4_weight(w):
    p = ops.nvfp4_amax_scale(w)
    q, s = ops.nvfp4_quantize(w, p)
    return q, s, p


def prepare(w, kind):
    """The tensors a family's call takes, from a bf16 weight."""
    if kind == "nvfp4":
        return nvfp4_weight(w)
    if kind == "int4":
        return ops.int4_quantize_tinygemm(w, 128)
    if kind == "mxfp4":
        return ops.mx_quantize(w, ops.MX_FMT_E2M1, "rceil")
    return (w,)


FAMILIES = {
    # name: (weight kind, call)
    "nvfp4_wo": ("nvfp4", lambda x, q, s, p: ops.nvfp4_wo_linear(x, q, s, p)),
    "nvfp4_dyn": ("nvfp4", lambda x, q, s, p: ops.nvfp4_linear(x, q, s, p, dynamic_per_tensor_scale=True)),
    "int4": ("int4", lambda x, q, sz: ops.weight_int4pack_mm(x, q, 128, sz)),
    "mxfp4": ("mxfp4", lambda x, q, s: ops.mx_linear(x, q, s, None, ops.MX_FMT_E2M1, "rceil")),
    "bf16": ("bf16", lambda x, w: F.linear(x, w)),
}


class Linears:
    def __init__(self, dev, layers, shapes, family):
        kind, self.call = FAMILIES[family]
        self.weights = []
        g = torch.Generator(device=dev).manual_seed(0)
        for _ in range(layers):
            for name, n, k in shapes:
                w = torch.randn(n, k, device=dev, dtype=torch.bfloat16, generator=g) * 0.02
                self.weights.append((k,) + tuple(prepare(w, kind)))
                del w
        self.x = {}
        self.bytes = sum(t.numel() * t.element_size() for w in self.weights for t in w[1:] if t.numel() > 1)

    def step(self, batch):
        for k, *w in self.weights:
            if (batch, k) not in self.x:
                self.x[(batch, k)] = torch.randn(batch, k, device=w[0].device, dtype=torch.bfloat16)
            self.call(self.x[(batch, k)], *w)


def graph_time(fn, stream, steps, warmup):
    with torch.cuda.stream(stream):  # (the int4 mm reserves its split-K workspace per stream: once outside the capture, on its stream)
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
    for family in ("nvfp4_wo", "nvfp4_dyn"):
        for other in ("bf16", "int4", "mxfp4"):
            res[family]["vs_" + other] = res[family]["tok_s"] / res[other]["tok_s"]
    res["route_bs1"] = {name: ops.nvfp4_linear_route(ops.NVFP4_KIND_WEIGHT_ONLY, 1, n, k) for name, n, k in bench.LLAMA3_8B_UNMERGED}
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
    """wo: the weight-only linear; dyn: the codes x codes GEMM alone, on an activation cast once (the cast is the same under both forms)."""
    for name, n, k in bench.LLAMA3_8B_UNMERGED:
        copies = max(2, -(-COLD_BYTES // (n * k * 9 // 16)))
        ws = []
        for _ in range(copies):
            w = torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.02
            ws.append(nvfp4_weight(w))
            del w
        reps = max(args.reps, 2 * copies)
        for m in SWEEP_M:
            x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
            pa = ops.nvfp4_amax_scale(x)
            a, a_s = ops.nvfp4_quantize(x, pa)
            r = {"sweep": name, "M": m, "N": n, "K": k, "copies": copies, "reps": reps}
            calls = {"wo": lambda i: ops.nvfp4_wo_linear(x, *ws[i]), "dyn": lambda i: ops.nvfp4_mm(a, a_s, ws[i][0], ws[i][1], pa, ws[i][2])}
            for kind, kid in (("wo", ops.NVFP4_KIND_WEIGHT_ONLY), ("dyn", ops.NVFP4_KIND_DYNAMIC)):
                r[f"{kind}_route"] = ops.nvfp4_linear_route(kid, m, n, k)["kernel"]
                for form, fname in ((1, "stream"), (2, "tile")):
                    ops.nvfp4_set_form(form)
                    try:
                        r[f"{kind}_{fname}_us"] = time_us(calls[kind], copies, reps)
                    finally:
                        ops.nvfp4_set_form(0)
            print(json.dumps(r), flush=True)
            if out:
                out.write(json.dumps(r) + "\n")
                out.flush()
        del ws
        torch.cuda.empty_cache()


def fit(path, out=None):
    """The hand-off row count per kind from a sweep file: the seam s (stream up to s rows, tiled beyond) with the least time summed over
    the five shapes and every swept M; per candidate the sum, so that the margin shows."""
    rows = [r for r in (json.loads(l) for l in open(path) if l.strip()) if "sweep" in r]
    ms = sorted({r["M"] for r in rows})
    for kind in ("wo", "dyn"):
        total = {}
        for seam in [0] + ms:
            total[seam] = sum(r[f"{kind}_stream_us"] if r["M"] <= seam else r[f"{kind}_tile_us"] for r in rows)
        best = min(total, key=total.get)
        line = json.dumps({"fit": kind, "seam": best, "summed_us_by_seam": {str(k): round(v, 1) for k, v in total.items()}})
        print(line)
        if out:
            out.write(line + "\n")


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
        sys.exit("bench_nvfp4_linear.py measures on the GPU: no device visible")
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
        if args.out:
            out.flush()
            fit(args.out, out)


if __name__ == "__main__":
    main()
