#!/usr/bin/env python3
"""The Intx linear measured, everything in this one process:
  * decode: one token (bs = 1) through the Llama-3-8B five-shape x LAYERS-layer linears, cold weights (every layer its own weights, more
    than the last-level cache in all), hipGraph replay: the fused linear on b-bit PACKED codes for b in {2, 3, 4, 6, 8} at group 64, the same
    tensor in its 8-bit container (unpacked, read in place), the reference's path (dequantize, then bf16 F.linear), int4 (tinygemm layout,
    group 128), int8 weight-only and PyTorch's bf16 F.linear; tok/s and the weight bytes (b / 8 a weight plus scale and zero-point) per
    second as a fraction of 8 TB/s;
  * --sweep: M over SWEEP_M on the five shapes, us per linear for both forms forced, at b = 4, the weight rotated through copies worth
    COLD_BYTES; then the `fit` line: the five shapes' time summed over every swept M per candidate seam.
    python tools/bench_intx_linear.py [--steps 20] [--sweep] [--out profiles/intx_linear.jsonl]"""
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
SWEEP_M = (1, 8, 16, 17, 32, 33, 48, 64, 65, 96, 128, 256)
COLD_BYTES = 512 << 20
GROUP = 64
BITS = (2, 3, 4, 6, 8)


def intx_weight(w, b, packed):
    q, s, zp = ops.intx_quantize(w, GROUP, b, "ASYMMETRIC")
    return (ops.intx_pack(q, b) if packed else q), s, zp


def families():
    fam = {}
    for b in BITS:
        fam[f"intx{b}_packed"] = (lambda w, b=b: intx_weight(w, b, True), lambda x, q, s, zp, b=b: ops.intx_linear(x, q, s, zp, b))
        fam[f"intx{b}_unpacked"] = (lambda w, b=b: intx_weight(w, b, False), lambda x, q, s, zp, b=b: ops.intx_linear(x, q, s, zp, b))
    fam["intx4_dequantize_linear"] = (lambda w: intx_weight(w, 4, False), lambda x, q, s, zp: F.linear(x, ops.intx_dequantize(q, s, zp, 4)))
    fam["int4"] = (lambda w: ops.int4_quantize_tinygemm(w, 128), lambda x, q, sz: ops.weight_int4pack_mm(x, q, 128, sz))
    fam["int8_wo"] = (ops.int8_quantize_rowwise, lambda x, q, s: ops.int8_wo_linear(x, q, s))
    fam["bf16"] = (lambda w: (w,), lambda x, w: F.linear(x, w))
    return fam


class Linears:
    def __init__(self, dev, layers, shapes, prepare, call):
        self.call, self.weights, self.x = call, [], {}
        g = torch.Generator(device=dev).manual_seed(0)
        for _ in range(layers):
            for _, n, k in shapes:
                w = torch.randn(n, k, device=dev, dtype=torch.bfloat16, generator=g) * 0.02
                self.weights.append((k,) + tuple(prepare(w)))
                del w
        self.bytes = sum(t.numel() * t.element_size() for w in self.weights for t in w[1:])

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


def decode(args, dev, emit):
    stream = torch.cuda.Stream(device=dev)
    with torch.no_grad():
        for name, (prepare, call) in families().items():
            m = Linears(dev, args.layers, bench.LLAMA3_8B_UNMERGED, prepare, call)
            sec = graph_time(lambda: m.step(1), stream, args.steps, args.warmup)
            emit({"decode": name, "layers": args.layers, "tok_s": 1.0 / sec, "step_us": sec * 1e6, "weight_bytes": m.bytes,
                  "hbm_fraction": m.bytes / sec / HBM_BPS})
            del m
            torch.cuda.empty_cache()


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


def sweep(args, dev, emit, b=4):
    total = {}
    for name, n, k in bench.LLAMA3_8B_UNMERGED:
        copies = max(2, -(-COLD_BYTES // (n * k * b // 8)))
        ws = []
        for _ in range(copies):
            w = torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.02
            ws.append(intx_weight(w, b, True))
            del w
        for m in SWEEP_M:
            x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
            row = {"sweep": name, "N": n, "K": k, "M": m, "bits": b, "copies": copies}
            for form, key in ((1, "stream_us"), (2, "tile_us")):
                ops.intx_linear_set_form(form)
                try:
                    row[key] = min(time_us(lambda i: ops.intx_linear(x, *ws[i], b), copies, max(args.reps, 2 * copies)) for _ in range(2))
                finally:
                    ops.intx_linear_set_form(0)
                total[(m, key)] = total.get((m, key), 0.0) + row[key]
            emit(row)
        del ws
        torch.cuda.empty_cache()
    # per candidate seam: the stream form up to it, the tiled form beyond, the five shapes summed over every swept M
    fit = {str(seam): sum(total[(m, "stream_us" if m <= seam else "tile_us")] for m in SWEEP_M) for seam in (0,) + SWEEP_M}
    emit({"fit": fit, "best_seam": int(min(fit, key=fit.get)), "bits": b})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = open(args.out, "a") if args.out else None

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    (sweep if args.sweep else decode)(args, dev, emit)


if __name__ == "__main__":
    main()
