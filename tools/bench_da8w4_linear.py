#!/usr/bin/env python3
"""W4A8 linears, everything in this one process:
  * decode: one token (bs = 1) through the Llama-3-8B five shapes x --layers layers (every layer its own weights: cold, more than the
    last-level cache in all), one captured graph a family, replayed: W4A8 (cast + GEMM a linear) at g = 128 and g = 32, the int4 weight-only
    linear, the int8 dynamic linear and bf16 F.linear;
  * rows: M = 16 .. 4096 on o and gate next to the same three, and the tiled form's share of the int8 MFMA peak per group size;
  * --sweep: both forms forced over M and the fitted seam (the last swept M up to which the stream form is ahead, summed over the shapes).
Rows and sweep: operands rotate through copies worth 512 MiB; device events around windows of calls, the families of a cell alternating;
the median over --replays windows and (max - min) / median as the spread.  One JSON line per cell.
    python tools/bench_da8w4_linear.py [--sweep] [--replays 5] [--layers 32] [--out profiles/da8w4_linear.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
from ao_amd import ops  # noqa: E402

COLD_BYTES = 512 << 20
WINDOW_US = 20e3
INT8_PEAK_TOPS = 4600.0  # MI355X dense int8, the figure the share of peak is taken against
ROWS = (16, 64, 256, 1024, 4096)
SWEEP_M = (1, 8, 16, 32, 48, 64, 96, 128, 256)
DEV = torch.device("cuda", 0)


def one_window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def alternate(fns, replays):
    calls = []
    for fn in fns.values():
        one_window(fn, 3)
        calls.append(max(5, min(400, int(WINDOW_US / max(one_window(fn, 5), 1e-3)))))
    times = {name: [] for name in fns}
    for _ in range(replays):
        for name, fn in fns.items():
            times[name].append(one_window(fn, min(calls)))
    return {name: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for name, t in times.items()}


def copies(nbytes):
    return max(2, min(64, -(-COLD_BYTES // nbytes)))


def emit(out, rec, r, base=None):
    for k, (us, spread) in r.items():
        rec[k + "_us"], rec[k + "_spread"] = round(us, 2), round(spread, 4)
    if base:
        rec.update({f"da8w4_vs_{k}": round(r[k][0] / r[base][0], 3) for k in r if k != base and not k.startswith("da8w4")})
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")


def decode_families():
    """name -> (prepare(w) -> the weight's tensors, call(x, *tensors))"""
    fam = {}
    for g in (128, 32):
        fam[f"da8w4_g{g}"] = (lambda w, g=g: ops.da8w4_quantize_weight(w, g)[:2], lambda x, q, sz: ops.da8w4_linear(x, q, sz))
    fam["int4"] = (lambda w: ops.int4_quantize_tinygemm(w, 128), lambda x, q, sz: ops.weight_int4pack_mm(x, q, 128, sz))
    fam["int8_dynamic"] = (ops.int8_quantize_rowwise, lambda x, q, s: ops.int8_linear(x, q, s))
    fam["bf16"] = (lambda w: (w,), lambda x, w: F.linear(x, w))
    return fam


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
    times = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / steps)
    return statistics.median(times), (max(times) - min(times)) / statistics.median(times)


def decode(out, layers):
    stream = torch.cuda.Stream(device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(0)
    xs = {k: torch.randn(1, k, device=DEV, dtype=torch.bfloat16) for k in (4096, 14336)}
    res = {}
    for name, (prepare, call) in decode_families().items():
        weights = []
        for _ in range(layers):
            for _, n, k in bench.LLAMA3_8B_UNMERGED:
                weights.append((k,) + tuple(prepare(torch.randn(n, k, device=DEV, dtype=torch.bfloat16, generator=gen) * 0.02)))

        def step():
            for k, *w in weights:
                call(xs[k], *w)

        res[name] = graph_time(step, stream, 20, 5)
        nbytes = sum(t.numel() * t.element_size() for w in weights for t in w[1:])
        emit(out, {"cell": "decode_graph", "family": name, "layers": layers, "linears": len(weights), "weight_bytes": nbytes,
                   "step_us": round(res[name][0], 1), "spread": round(res[name][1], 4), "us_per_linear": round(res[name][0] / len(weights), 2),
                   "weight_tbps": round(nbytes / res[name][0] * 1e-6, 3)}, {})
        del weights
        torch.cuda.empty_cache()
    emit(out, {"cell": "decode_graph_ratios", **{f"{a}_vs_{b}": round(res[b][0] / res[a][0], 3) for a in ("da8w4_g128", "da8w4_g32")
                                                  for b in ("int4", "int8_dynamic", "bf16")}}, {})


def families(n, k, g):
    """the weight of one shape in every family, each rotated through cold copies"""
    w = torch.randn(n, k, device=DEV, dtype=torch.bfloat16) * 0.02
    wa = [ops.da8w4_quantize_weight(w, g)[:2] for _ in range(copies(n * k // 2))]
    w4 = [ops.int4_quantize_tinygemm(w, 128) for _ in range(copies(n * k // 2))]
    w8 = [ops.int8_quantize_rowwise(w) for _ in range(copies(n * k))]
    wb = [w.clone() for _ in range(copies(2 * n * k))]
    return wa, w4, w8, wb


def cell(out, kind, name, m, n, k, g, replays):
    wa, w4, w8, wb = families(n, k, g)
    x = torch.randn(m, k, device=DEV, dtype=torch.bfloat16)
    act = ops.da8w4_quantize_act(x, g)
    act = (act[0], act[1], act[3])
    r = alternate({"da8w4": lambda i: ops.da8w4_linear(x, *wa[i % len(wa)]),
                   "da8w4_mm": lambda i: ops.da8w4_linear(x, *wa[i % len(wa)], act=act),
                   "int4": lambda i: ops.weight_int4pack_mm(x, w4[i % len(w4)][0], 128, w4[i % len(w4)][1]),
                   "int8_dynamic": lambda i: ops.int8_linear(x, *w8[i % len(w8)]),
                   "bf16": lambda i: F.linear(x, wb[i % len(wb)])}, replays)
    tops = 2.0 * m * n * k / r["da8w4_mm"][0] * 1e-6
    emit(out, {"cell": kind, "shape": name, "M": m, "N": n, "K": k, "g": g, "kernel": ops.da8w4_linear_kernel_name(m, n, k, g),
               "da8w4_mm_tops": round(tops, 1), "da8w4_mm_share_of_int8_peak": round(tops / INT8_PEAK_TOPS, 4),
               "da8w4_mm_weight_tbps": round(n * k / 2 / r["da8w4_mm"][0] * 1e-6, 3)}, r, "da8w4")


def sweep(out, replays):
    total = {m: [0.0, 0.0] for m in SWEEP_M}
    for name, n, k in (("o", 4096, 4096), ("gate", 14336, 4096)):
        wa = [ops.da8w4_quantize_weight(torch.randn(n, k, device=DEV, dtype=torch.bfloat16) * 0.02, 128)[:2] for _ in range(copies(n * k // 2))]
        for m in SWEEP_M:
            x = torch.randn(m, k, device=DEV, dtype=torch.bfloat16)
            act = ops.da8w4_quantize_act(x, 128)
            act = (act[0], act[1], act[3])

            def forced(form):
                def run(i):
                    ops.da8w4_linear_set_form(form)
                    ops.da8w4_linear(x, *wa[i % len(wa)], act=act)
                return run

            r = alternate({"stream": forced(1), "tiled": forced(2)}, replays)
            ops.da8w4_linear_set_form(0)
            total[m][0] += r["stream"][0]
            total[m][1] += r["tiled"][0]
            emit(out, {"cell": "forms", "shape": name, "M": m, "N": n, "K": k, "g": 128}, r)
    ahead = [m for m in SWEEP_M if total[m][1] < total[m][0]]
    last = max((m for m in SWEEP_M if all(t not in ahead for t in SWEEP_M if t <= m)), default=0)
    emit(out, {"cell": "fit", "sum_over_shapes_us": {str(m): [round(v, 1) for v in t] for m, t in total.items()},
               "last_M_up_to_which_stream_is_ahead": last, "route_seam": max(m for m in range(1, 513) if ops.da8w4_linear_route(m, 4096, 4096, 128)["kernel"] == "da8w4_stream_kernel")}, {})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "da8w4_linear.jsonl"))
    args = ap.parse_args()
    with open(args.out, "w") as out, torch.no_grad():
        decode(out, args.layers)
        for name, n, k in (("o", 4096, 4096), ("gate", 14336, 4096)):
            for m in ROWS:
                for g in ((32, 64, 128) if m == 4096 else (128,)):
                    cell(out, "rows", name, m, n, k, g, args.replays)
        if args.sweep:
            sweep(out, args.replays)


if __name__ == "__main__":
    main()
