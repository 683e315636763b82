#!/usr/bin/env python3
"""The NVFP4 grouped GEMM measured on one EP-8 rank's experts, the cells of tools/bench_fp8_block_grouped.py so that
the two tables read side by side:

    model             E    gate_up [N, K]   down [N, K]
    DeepSeek-V3       32   [4096, 7168]     [7168, 2048]
    Qwen3-235B-A22B   16   [3072, 4096]     [4096, 1536]

Row sets: 64 rows spread over the experts by a seeded multinomial (decode), 16 / 128 / 512 rows on every expert.
Per cell and kind (wo: bf16 activations x NVFP4 weights; dyn: codes x codes with per-group and per-expert scales), in this one process and
under the same hipGraph (the weights rotated through copies worth 512 MB so that they come from HBM, one call per copy in the graph, the
median of the replays):
  * grouped_us: ops.nvfp4_grouped_mm alone; hbm_fraction: the bytes of the experts hit (codes and block scales) per second as a share of
    8 TB/s; (dyn) cast_grouped_us: the per-group amax, the grouped cast, then the GEMM;
  * loop_us: a loop of ops.nvfp4_wo_linear / ops.nvfp4_mm over the non-empty groups (one launch per expert hit: what the library offered
    before the grouped entry);
  * fp8_block_us: ops.fp8_block_grouped_mm on the same shapes (records of the wo kind);
  * bf16_eager_us (records of their own, measured last): torch._grouped_mm on the experts dequantized to bf16, EAGER calls (launch gaps
    included) -- what the reference's emulation costs after its two dequantizations.
--sweep: each form forced (ao_nvfp4_grouped_mm_set_form) over uniform groups of 2 .. 512 rows on the four shapes, both kinds; --fit FILE
prints the hand-over (stream up to s rows of mean group size, tiled beyond) with the least summed time of a results file, and the decode
cells in which the grouped launch was not faster than the loop (no GPU).
    python tools/bench_nvfp4_grouped.py [--replays 7] [--sweep] [--no-cells] [--no-bf16 | --bf16-only] [--shapes NAME,...] [--tag LABEL]
                                        [--decode-only] [--form 0|1|2] [--out profiles/nvfp4_grouped.jsonl]"""
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
# (the blockwise tool's group sizes, and 2 / 4 / 8 rows below them: the first fit put the hand-over below 16 rows)
SWEEP_ROWS = (2, 4, 8, 16, 32, 48, 64, 96, 128, 160, 192, 256, 384, 512)
DECODE_SETS = ("decode64", "each16")
KINDS = (("wo", ops.NVFP4_KIND_WEIGHT_ONLY), ("dyn", ops.NVFP4_KIND_DYNAMIC))
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
    """`copies` sets of E experts [N, K] in NVFP4 under per-expert scales (the device amax and the grouped cast over the [E N, K] view)
    and, with_block, the blockwise float8 cast of the same bf16 weights."""

    def __init__(self, dev, e, n, k, with_block):
        self.copies = max(1, -(-COLD_BYTES // (e * n * (k // 2 + k // 16))))
        self.nv, self.block = [], []
        woffs = (torch.arange(1, e + 1, device=dev) * n).to(torch.int32)
        for _ in range(self.copies):
            w = (torch.randn(e, n, k, device=dev, dtype=torch.bfloat16) * 0.02).reshape(e * n, k)
            p = ops.nvfp4_group_amax_scale(w, woffs)
            q, s = ops.nvfp4_quantize_grouped(w, p, woffs)
            self.nv.append((q.reshape(e, n, k // 2), s.reshape(e, n, k // 16), p))
            if with_block:
                bq, bs = ops.fp8_quantize_block_128x128(w)
                self.block.append((bq.reshape(e, n, k), bs.reshape(e, n // 128, k // 128)))
            del w


def cell(dev, stream, ex, name, e, n, k, set_name, sizes, replays, kind_name, kind):
    m = sum(sizes)
    offs_host = torch.tensor(sizes).cumsum(0)
    offs = offs_host.to(torch.int32).to(dev)
    bounds = [(i, int(offs_host[i]) - sizes[i], int(offs_host[i])) for i in range(e) if sizes[i] > 0]
    x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
    pa = ops.nvfp4_group_amax_scale(x, offs)
    aq, a_s = ops.nvfp4_quantize_grouped(x, pa, offs)
    pas = [pa[g] for g, _, _ in bounds]
    out = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
    hit_bytes = len(bounds) * n * (k // 2 + k // 16)
    r = {"cell": name, "kind": kind_name, "rows": set_name, "E": e, "N": n, "K": k, "M_total": m, "experts_hit": len(bounds),
         "copies": ex.copies, "replays": replays, "route": ops.nvfp4_grouped_mm_route(kind, m, n, k, e)}
    if kind_name == "wo":
        def grouped(i):
            q, s, p = ex.nv[i]
            ops.nvfp4_grouped_mm(kind, x, None, q, s, offs, None, p, out=out)

        def loop(i):
            q, s, p = ex.nv[i]
            for g, b, t in bounds:
                ops.nvfp4_wo_linear(x[b:t], q[g], s[g], p[g], out=out[b:t])
    else:
        def grouped(i):
            q, s, p = ex.nv[i]
            ops.nvfp4_grouped_mm(kind, aq, a_s, q, s, offs, pa, p, out=out)

        def cast_grouped(i):
            q, s, p = ex.nv[i]
            pg = ops.nvfp4_group_amax_scale(x, offs)
            cq, cs = ops.nvfp4_quantize_grouped(x, pg, offs)
            ops.nvfp4_grouped_mm(kind, cq, cs, q, s, offs, pg, p, out=out)

        def loop(i):
            q, s, p = ex.nv[i]
            for j, (g, b, t) in enumerate(bounds):
                ops.nvfp4_mm(aq[b:t], a_s[b:t], q[g], s[g], pas[j], p[g], out=out[b:t])

    r["grouped_us"] = graph_us(grouped, ex.copies, stream, replays)
    r["hbm_fraction"] = hit_bytes / (r["grouped_us"] * 1e-6) / HBM_BPS
    if kind_name == "dyn":
        r["cast_grouped_us"] = graph_us(cast_grouped, ex.copies, stream, replays)
    r["loop_us"] = graph_us(loop, ex.copies, stream, replays)
    r["grouped_vs_loop"] = r["loop_us"] / r["grouped_us"]
    if kind_name == "wo" and ex.block:
        bq, bs = ops.fp8_quantize_block_1x128(x)
        r["fp8_block_us"] = graph_us(lambda i: ops.fp8_block_grouped_mm(bq, bs, *ex.block[i % len(ex.block)], offs, out=out), ex.copies, stream,
                                     replays)
    return r


def shapes_of(args):
    want = set(args.shapes.split(",")) if args.shapes else None
    return [s for s in SHAPES if want is None or s[0] in want]


def cells(args, dev, out):
    stream = torch.cuda.Stream(device=dev)
    for name, e, n, k in shapes_of(args):
        ex = Experts(dev, e, n, k, with_block=True)
        sets = row_sets(e)
        for set_name in (DECODE_SETS if args.decode_only else sets):
            for kind_name, kind in KINDS:
                emit(cell(dev, stream, ex, name, e, n, k, set_name, sets[set_name], args.replays, kind_name, kind), out)
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
    """The bf16 torch._grouped_mm column, after everything else, eager: the GEMM of the reference's emulation on experts that are already
    dequantized (2 bytes a weight), its dequantizations left out."""
    for name, e, n, k in shapes_of(args):
        copies = max(1, -(-COLD_BYTES // (2 * e * n * k)))
        ws = [torch.randn(e, n, k, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(copies)]
        for set_name, sizes in row_sets(e).items():
            x = torch.randn(sum(sizes), k, device=dev, dtype=torch.bfloat16)
            offs = torch.tensor(sizes).cumsum(0).to(torch.int32).to(dev)
            r = {"bf16_cell": name, "rows": set_name, "E": e, "N": n, "K": k, "copies": copies, "replays": args.replays}
            r["bf16_eager_us"] = eager_us(lambda i: torch._grouped_mm(x, ws[i].transpose(-2, -1), offs=offs, out_dtype=torch.bfloat16), copies,
                                          args.replays)
            emit(r, out)
        del ws
        torch.cuda.empty_cache()


def sweep(args, dev, out):
    stream = torch.cuda.Stream(device=dev)
    for name, e, n, k in shapes_of(args):
        ex = Experts(dev, e, n, k, with_block=False)
        for rows in SWEEP_ROWS:
            m = rows * e
            offs = (torch.arange(1, e + 1) * rows).to(torch.int32).to(dev)
            x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
            pa = ops.nvfp4_group_amax_scale(x, offs)
            aq, a_s = ops.nvfp4_quantize_grouped(x, pa, offs)
            o = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
            for kind_name, kind in KINDS:
                r = {"sweep": name, "kind": kind_name, "rows": rows, "E": e, "N": n, "K": k, "copies": ex.copies, "replays": args.replays,
                     "route": ops.nvfp4_grouped_mm_kernel_name(kind, m, n, k, e)}
                if kind_name == "wo":
                    fn = lambda i: ops.nvfp4_grouped_mm(kind, x, None, ex.nv[i][0], ex.nv[i][1], offs, None, ex.nv[i][2], out=o)  # noqa: E731
                else:
                    fn = lambda i: ops.nvfp4_grouped_mm(kind, aq, a_s, ex.nv[i][0], ex.nv[i][1], offs, pa, ex.nv[i][2], out=o)  # noqa: E731
                for form, fname in ((1, "stream"), (2, "tile")):
                    ops.nvfp4_grouped_mm_set_form(form)
                    try:
                        r[f"{fname}_us"] = graph_us(fn, ex.copies, stream, args.replays)
                    finally:
                        ops.nvfp4_grouped_mm_set_form(0)
                emit(r, out)
        del ex
        torch.cuda.empty_cache()


def fit(path):
    """From a results file: the seam s (stream up to s rows of mean group size, tiled beyond) with the least time summed over the four
    shapes, both kinds and every swept group size (and per kind); and the decode cells of the weight-only kind in which the grouped launch
    was not faster than the loop."""
    rows = [json.loads(l) for l in open(path) if l.strip()]
    rows = [r for r in rows if "fit" not in r]
    sw = [r for r in rows if "sweep" in r]
    if sw:
        ms = sorted({r["rows"] for r in sw})

        def totals(sel):
            return {seam: sum(r["stream_us"] if r["rows"] <= seam else r["tile_us"] for r in sel) for seam in [0] + ms}

        total = totals(sw)
        rec = {"fit": "seam", "seam": min(total, key=total.get), "summed_us_by_seam": {str(k): round(v, 1) for k, v in total.items()}}
        for kind in sorted({r["kind"] for r in sw}):
            t = totals([r for r in sw if r["kind"] == kind])
            rec[f"seam_{kind}"] = min(t, key=t.get)
            rec[f"summed_us_by_seam_{kind}"] = {str(k): round(v, 1) for k, v in t.items()}
        print(json.dumps(rec))
    ce = [r for r in rows if "cell" in r and r["rows"] in DECODE_SETS and r["kind"] == "wo"]
    if ce:
        slower = [(r["cell"], r["rows"], round(r["grouped_us"], 1), round(r["loop_us"], 1)) for r in ce if r["grouped_us"] >= r["loop_us"]]
        print(json.dumps({"fit": "decode_time_condition", "cells": len(ce), "grouped_not_faster_than_loop": slower,
                          "grouped_vs_loop": {f"{r['cell']}/{r['rows']}": round(r["grouped_vs_loop"], 2) for r in ce}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=7, help="graph replays per cell (the median is recorded; at least 5)")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-cells", action="store_true")
    ap.add_argument("--decode-only", action="store_true", help="only the two decode row sets of the cells")
    ap.add_argument("--no-bf16", action="store_true", help="skip the bf16 torch._grouped_mm records")
    ap.add_argument("--bf16-only", action="store_true", help="with --no-cells: only the bf16 torch._grouped_mm records (a run of their own)")
    ap.add_argument("--shapes", default=None, help="comma-separated shape names (default: all four)")
    ap.add_argument("--form", type=int, default=0, choices=(0, 1, 2), help="force a form on the cells' grouped launches (0: the product route)")
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
        sys.exit("bench_nvfp4_grouped.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None
    with torch.no_grad():
        if not args.no_cells:
            ops.nvfp4_grouped_mm_set_form(args.form)
            try:
                cells(args, dev, out)
            finally:
                ops.nvfp4_grouped_mm_set_form(0)
        if args.sweep:
            sweep(args, dev, out)
        if args.bf16_only or not (args.no_cells or args.no_bf16):
            bf16_cells(args, dev, out)


if __name__ == "__main__":
    main()
