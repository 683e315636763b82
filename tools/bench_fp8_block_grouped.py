#!/usr/bin/env python3
"""The blockwise float8 grouped GEMM measured on one EP-8 rank's experts:

    model             E    gate_up [N, K]   down [N, K]
    DeepSeek-V3       32   [4096, 7168]     [7168, 2048]
    Qwen3-235B-A22B   16   [3072, 4096]     [4096, 1536]

(gate and up merged into one tensor: the intermediate size is a multiple of 128, so no 128 x 128 block straddles the two.)
Row sets: 64 rows spread over the experts by a seeded multinomial (decode), 16 / 128 / 512 rows on every expert.
Per cell, in this one process and under the same hipGraph (the weights rotated through copies worth 512 MB so that they come from HBM,
one call per copy in the graph, the median of the replays):
  * grouped_us: ops.fp8_block_grouped_mm alone; cast_grouped_us: the 1 x 128 cast over all rows, then the GEMM; hbm_fraction: the bytes
    of the experts hit (codes and scales) per second of the GEMM alone as a share of 8 TB/s;
  * loop_us: a loop of ops.fp8_block_mm over the non-empty groups (one launch per expert hit: what the library offered before);
  * rowwise_us: the rowwise ops.fp8_grouped_mm on the same shapes (its output is zero-filled inside: one more fill than the others);
  * bf16_eager_us (records of their own, measured last): torch._grouped_mm on bf16 operands, EAGER calls (launch gaps included); one
    attempt under a graph follows (bf16_us: null with the error text where the installed torch cannot capture it).
--sweep: each form forced (ao_fp8_block_grouped_mm_set_form) over uniform groups of 16 .. 512 rows on the four shapes; --fit FILE prints
the hand-over (stream up to s rows of mean group size, tiled beyond) with the least summed time of a results file (no GPU).
    python tools/bench_fp8_block_grouped.py [--replays 7] [--sweep] [--no-cells] [--no-bf16 | --bf16-only] [--tag LABEL] [--out profiles/fp8_block_grouped.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ao_amd import ops  # noqa: E402

HBM_BPS = 8.0e12  # MI355X HBM3E peak
COLD_BYTES = 512 << 20  # rotate a cell's experts through copies worth this much: twice the last-level cache
SHAPES = [("deepseek_v3_gate_up", 32, 4096, 7168), ("deepseek_v3_down", 32, 7168, 2048),
          ("qwen3_235b_gate_up", 16, 3072, 4096), ("qwen3_235b_down", 16, 4096, 1536)]
SWEEP_ROWS = (16, 32, 48, 64, 96, 128, 160, 192, 256, 384, 512)
DECODE_SETS = ("decode64", "each16")
TAG = None


def row_sets(e):
    g = torch.Generator().manual_seed(e)
    hit = torch.multinomial(torch.ones(e), 64, replacement=True, generator=g)
    return {"decode64": torch.bincount(hit, minlength=e).tolist(), "each16": [16] * e, "each128": [128] * e, "each512": [512] * e}


def emit(r, out):
    if TAG:
        r = {"tag": TAG, **r}
    print(json.dumps(r), flush=True)
    if out:
        out.write(json.dumps(r) + "\n")
        out.flush()


def graph_us(fn, copies, stream, replays):
    """Median over the replays of a graph that holds one call per weight copy, per call."""
    for i in range(copies):
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            for i in range(copies):
                fn(i)
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / copies)
    return statistics.median(times)


class Experts:
    """`copies` sets of E experts [N, K]: blockwise and rowwise float8 casts of the same bf16 weights."""

    def __init__(self, dev, e, n, k):
        self.copies = max(1, -(-COLD_BYTES // (e * n * k)))
        self.block, self.row = [], []
        for _ in range(self.copies):
            w = torch.randn(e, n, k, device=dev, dtype=torch.bfloat16) * 0.02
            q, s = ops.fp8_quantize_block_128x128(w.reshape(e * n, k))
            self.block.append((q.reshape(e, n, k), s.reshape(e, n // 128, k // 128)))
            rq, rs = ops.fp8_quantize_rowwise(w.reshape(e * n, k))
            self.row.append((rq.reshape(e, n, k), rs.reshape(e, n)))
            del w


def cell(dev, stream, ex, name, e, n, k, set_name, sizes, replays):
    m = sum(sizes)
    offs_host = torch.tensor(sizes).cumsum(0)
    offs = offs_host.to(torch.int32).to(dev)
    bounds = [(i, int(offs_host[i]) - sizes[i], int(offs_host[i])) for i in range(e) if sizes[i] > 0]
    x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
    aq, a_s = ops.fp8_quantize_block_1x128(x)
    rq, rs = ops.fp8_quantize_rowwise(x)
    out = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
    hit_bytes = len(bounds) * (n * k + 4 * (n // 128) * (k // 128))
    r = {"cell": name, "rows": set_name, "E": e, "N": n, "K": k, "M_total": m, "experts_hit": len(bounds), "copies": ex.copies, "replays": replays,
         "route": ops.fp8_block_grouped_mm_route(m, n, k, e)}

    def grouped(i):
        ops.fp8_block_grouped_mm(aq, a_s, *ex.block[i], offs, out=out)

    def cast_grouped(i):
        q, s = ops.fp8_quantize_block_1x128(x)
        ops.fp8_block_grouped_mm(q, s, *ex.block[i], offs, out=out)

    def loop(i):
        wq, ws = ex.block[i]
        for g, b, t in bounds:
            ops.fp8_block_mm(aq[b:t], a_s[b:t], wq[g], ws[g], out=out[b:t])

    def rowwise(i):
        ops.fp8_grouped_mm(rq, rs, *ex.row[i], offs)

    r["grouped_us"] = graph_us(grouped, ex.copies, stream, replays)
    r["cast_grouped_us"] = graph_us(cast_grouped, ex.copies, stream, replays)
    r["hbm_fraction"] = hit_bytes / (r["grouped_us"] * 1e-6) / HBM_BPS
    r["loop_us"] = graph_us(loop, ex.copies, stream, replays)
    r["rowwise_us"] = graph_us(rowwise, ex.copies, stream, replays)
    r["grouped_vs_loop"] = r["loop_us"] / r["grouped_us"]
    return r


def cells(args, dev, out):
    stream = torch.cuda.Stream(device=dev)
    for name, e, n, k in SHAPES:
        ex = Experts(dev, e, n, k)
        for set_name, sizes in row_sets(e).items():
            emit(cell(dev, stream, ex, name, e, n, k, set_name, sizes, args.replays), out)
        del ex
        torch.cuda.empty_cache()


def eager_us(fn, copies, replays):
    """Median over the replays of `copies` eager calls, per call (launch gaps included: for what cannot be captured)."""
    for i in range(copies):
        fn(i)
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(copies):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / copies)
    return statistics.median(times)


def bf16_cells(args, dev, out):
    """The bf16 torch._grouped_mm column, after everything else, eager first: a torch whose bf16 grouped mm cannot be captured fails
    inside the capture, and what a failed capture leaves behind must not touch the other columns.  The failure is recorded, not
    hidden, and the graph is not tried again after it."""
    stream = torch.cuda.Stream(device=dev)
    sets = [(name, e, n, k, set_name, sizes) for name, e, n, k in SHAPES for set_name, sizes in row_sets(e).items()]
    recs, weights = [], {}
    for name, e, n, k, set_name, sizes in sets:
        if name not in weights:
            weights.clear()
            torch.cuda.empty_cache()
            copies = max(1, -(-COLD_BYTES // (2 * e * n * k)))
            weights[name] = [torch.randn(e, n, k, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(copies)]
        ws = weights[name]
        x = torch.randn(sum(sizes), k, device=dev, dtype=torch.bfloat16)
        offs = torch.tensor(sizes).cumsum(0).to(torch.int32).to(dev)
        r = {"bf16_cell": name, "rows": set_name, "E": e, "N": n, "K": k, "copies": len(ws), "replays": args.replays}
        r["bf16_eager_us"] = eager_us(lambda i: torch._grouped_mm(x, ws[i].transpose(-2, -1), offs=offs, out_dtype=torch.bfloat16), len(ws),
                                      args.replays)
        if not recs:  # the first cell is tried under a graph at the end
            recs.append((r, x, offs, ws))
        emit(r, out)
    r, x, offs, ws = recs[0]
    g = {"bf16_graph": r["bf16_cell"], "rows": r["rows"]}
    try:
        g["bf16_us"] = graph_us(lambda i: torch._grouped_mm(x, ws[i].transpose(-2, -1), offs=offs, out_dtype=torch.bfloat16), len(ws), stream,
                                args.replays)
    except Exception as err:  # noqa: BLE001
        g["bf16_us"], g["bf16_error"] = None, f"{type(err).__name__}: {str(err)[:200]}"
    emit(g, out)


def sweep(args, dev, out):
    stream = torch.cuda.Stream(device=dev)
    for name, e, n, k in SHAPES:
        ex = Experts(dev, e, n, k)
        for rows in SWEEP_ROWS:
            m = rows * e
            offs = (torch.arange(1, e + 1) * rows).to(torch.int32).to(dev)
            aq, a_s = ops.fp8_quantize_block_1x128(torch.randn(m, k, device=dev, dtype=torch.bfloat16))
            o = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
            r = {"sweep": name, "rows": rows, "E": e, "N": n, "K": k, "copies": ex.copies, "replays": args.replays,
                 "route": ops.fp8_block_grouped_mm_kernel_name(m, n, k, e)}
            for form, fname in ((1, "stream"), (2, "tile")):
                ops.fp8_block_grouped_mm_set_form(form)
                try:
                    r[f"{fname}_us"] = graph_us(lambda i: ops.fp8_block_grouped_mm(aq, a_s, *ex.block[i], offs, out=o), ex.copies, stream,
                                                args.replays)
                finally:
                    ops.fp8_block_grouped_mm_set_form(0)
            emit(r, out)
        del ex
        torch.cuda.empty_cache()


def fit(path):
    """From a results file: the seam s (stream up to s rows of mean group size, tiled beyond) with the least time summed over the four
    shapes and every swept group size; and the decode cells in which the grouped launch was slower than the loop."""
    rows = [json.loads(l) for l in open(path) if l.strip()]
    sw = [r for r in rows if "sweep" in r]
    if sw:
        ms = sorted({r["rows"] for r in sw})
        total = {seam: sum(r["stream_us"] if r["rows"] <= seam else r["tile_us"] for r in sw) for seam in [0] + ms}
        print(json.dumps({"fit": "seam", "seam": min(total, key=total.get), "summed_us_by_seam": {str(k): round(v, 1) for k, v in total.items()}}))
    ce = [r for r in rows if "cell" in r and r["rows"] in DECODE_SETS]
    if ce:
        slower = [(r["cell"], r["rows"], round(r["grouped_us"], 1), round(r["loop_us"], 1)) for r in ce if r["grouped_us"] > r["loop_us"]]
        print(json.dumps({"fit": "decode_time_condition", "cells": len(ce), "grouped_slower_than_loop": slower}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=7, help="graph replays per cell (the median is recorded; at least 5)")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-cells", action="store_true")
    ap.add_argument("--no-bf16", action="store_true", help="skip the bf16 torch._grouped_mm records")
    ap.add_argument("--bf16-only", action="store_true", help="with --no-cells: only the bf16 torch._grouped_mm records (a run of their own)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default=None, help="a label written into every record of this run")
    ap.add_argument("--fit", default=None, metavar="JSONL", help="no GPU: print the fitted seam and the decode time condition of a results file")
    args = ap.parse_args()
    if args.fit:
        return fit(args.fit)
    if args.replays < 5:
        ap.error("--replays must be at least 5")
    global TAG
    TAG = args.tag
    if not torch.cuda.is_available():
        sys.exit("bench_fp8_block_grouped.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None
    with torch.no_grad():
        if not args.no_cells:
            cells(args, dev, out)
        if args.sweep:
            sweep(args, dev, out)
        if args.bf16_only or not (args.no_cells or args.no_bf16):
            bf16_cells(args, dev, out)


if __name__ == "__main__":
    main()
