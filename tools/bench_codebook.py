#!/usr/bin/env python3
"""The codebook (k-means) kernels measured, everything in this one process:
  * lloyd: one ops.codebook_lloyd_step per format on Llama-3-8B weight shapes next to the reference's iteration in eager ops (chunked
    addmm(beta=-0.5) + argmax + index_reduce_("mean", include_self=False)), on the same data and table;
  * from_float: CodebookQuantizedTensor.from_float whole (scales, farthest-point initialisation, k-means, codes) next to the same loop
    with the eager iteration, on one 1024 x 4096 weight;
  * decode: one token (bs = 1) through the Llama-3-8B five-shape x 32-layer linears, cold weights (every layer its own), hipGraph
    replay: the fused linear and dequantize + F.linear per format, int4 (tinygemm, group 128), NF4 and PyTorch's bf16 F.linear; tok/s and
    the weight bytes per second as a fraction of 8 TB/s.  A family whose 32 layers hold less than 512 MiB is measured over as many more
    layers as pass it (`layers_measured`), its time scaled back to 32;
  * gather: the fused linear with random codes next to equal codes (no LDS bank conflict): the most a replicated or skewed table could win;
  * --sweep: M = 1 .. 256 on the five shapes (uint8 codes, every block width), us per linear for the fused form (forced) and
    for dequantize + F.linear, the weights rotated through copies worth twice the last-level cache, WINDOWS windows a cell, then the
    `fit` line: the summed time per candidate seam (fastest window of each cell).
    python tools/bench_codebook.py [--steps 20] [--sweep] [--out profiles/codebook.jsonl]"""
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
from ao_amd.prototype import CodebookQuantizedTensor  # noqa: E402
from ao_amd.prototype import codebook as cb  # noqa: E402
from ao_amd.quantization import to_nf4  # noqa: E402

HBM_BPS = 8.0e12
FORMATS = [("uint8", 1, 256), ("uint4", 1, 16), ("uint8", 4, 256), ("uint8", 8, 256), ("uint4", 8, 16)]  # 8, 4, 2, 1, 0.5 bits a weight
SWEEP_M = (1, 2, 4, 8, 16, 17, 24, 32, 33, 48, 64, 65, 96, 128, 192, 256)
COLD_BYTES = 512 << 20
WINDOWS = 3
CHUNK_VALS = 2 ** 28  # scores of a chunk of the eager iteration (1 GiB of fp32; the reference's default of 2^30 does not fit beside the weights)


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


def windows(fn, copies, reps):
    return [time_us(fn, copies, reps) for _ in range(WINDOWS)]


def eager_iteration(data, table):
    """fit_kmeans' iteration as the reference runs it on one device"""
    k = table.shape[0]
    codes = torch.empty(len(data), dtype=torch.int64, device=data.device)
    half = torch.bmm(table[:, None, :], table[:, :, None]).flatten()
    step = CHUNK_VALS // k
    for s in range(0, len(data), step):
        codes[s:s + step] = torch.addmm(half, data[s:s + step], table.T, beta=-0.5).argmax(1)
    return table.clone().index_reduce_(0, codes, data, "mean", include_self=False)


def lloyd(dev, emit):
    for n, kk in ((4096, 4096), (14336, 4096)):
        w = torch.randn(n, kk, device=dev, dtype=torch.bfloat16) * 0.02
        for name, d, k in FORMATS:
            _, data = cb._scales_and_data(w, d, kk)
            table = data[torch.randperm(len(data), device=dev)[:k]].contiguous()
            r = {"lloyd": f"{n}x{kk}", "codes": name, "d": d, "k": k, "rows": len(data)}
            r["fused_us"] = windows(lambda i: ops.codebook_lloyd_step(data, table), 1, 5)
            r["eager_us"] = windows(lambda i: eager_iteration(data, table), 1, 2)
            r["speedup"] = min(r["eager_us"]) / min(r["fused_us"])
            r["fused_GFMA_per_s"] = len(data) * k * d / min(r["fused_us"]) / 1e3
            emit(r)
            del data
        del w
        torch.cuda.empty_cache()


def from_float(dev, emit):
    w = torch.randn(1024, 4096, device=dev, dtype=torch.bfloat16) * 0.02
    for name, d, k in (("uint4", 1, 16), ("uint8", 8, 256)):
        dtype = getattr(torch, name)

        def eager():
            _, data = cb._scales_and_data(w, d, 4096)
            table = cb._farthest_point_init(data, k)
            for i in range(200):
                new = eager_iteration(data, table)
                if i % 10 == 0 and torch.allclose(new, table, rtol=1e-6, atol=1e-8):
                    break
                table = new
            return i

        r = {"from_float": "1024x4096", "codes": name, "d": d, "k": k}
        r["fused_us"] = windows(lambda i: CodebookQuantizedTensor.from_float(w, (1, d), dtype, 4096), 1, 2)
        r["eager_loop_us"] = windows(lambda i: eager(), 1, 2)
        r["speedup"] = min(r["eager_loop_us"]) / min(r["fused_us"])
        emit(r)


# ---- decode ---------------------------------------------------------------------------------------------------------------------------------
def fields(w, d, k):
    """Random fields of the format (timing only: the kernels' time does not depend on the values)"""
    n, kk = w.shape
    codes = torch.randint(0, 256, (n, kk // d // (2 if k == 16 else 1)), device=w.device, dtype=torch.uint8)
    table = torch.randn(k, 1, d, device=w.device, dtype=torch.bfloat16)
    return codes, table, torch.rand(n, 1, 1, device=w.device, dtype=torch.bfloat16)


def _fused(x, n, k, *f):
    ops.codebook_linear_set_form(1)
    try:
        return ops.codebook_linear(x, *f)
    finally:
        ops.codebook_linear_set_form(0)


def _nf4(w):
    t = to_nf4(w, 64, 256)
    return t.quantized_data, t.quantized_scalers, t.quantization_factor, t.scaler_mean


FAMILIES = {f"codebook_{name}_d{d}": ((lambda w, d=d, k=k: fields(w, d, k)), _fused) for name, d, k in FORMATS}
FAMILIES.update({f"codebook_{name}_d{d}_dequantize_linear": ((lambda w, d=d, k=k: fields(w, d, k)), lambda x, n, k, *f: F.linear(x, ops.codebook_dequantize(*f)))
                 for name, d, k in FORMATS})
FAMILIES.update({
    "int4": (lambda w: ops.int4_quantize_tinygemm(w, 128), lambda x, n, k, q, sz: ops.weight_int4pack_mm(x, q, 128, sz)),
    "nf4": (_nf4, lambda x, n, k, *f: ops.nf4_linear(x, *f, n, k, 64, 256)),
    "bf16": (lambda w: (w,), lambda x, n, k, w: F.linear(x, w)),
})


class Linears:
    def __init__(self, dev, layers, shapes, family):
        prepare, self.call = FAMILIES[family]
        self.weights = []
        g = torch.Generator(device=dev).manual_seed(0)
        for _ in range(layers):
            for name, n, k in shapes:
                w = torch.randn(n, k, device=dev, dtype=torch.bfloat16, generator=g) * 0.02
                self.weights.append((n, k) + tuple(prepare(w)))
                del w
        self.x = {}
        self.bytes = sum(t.numel() * t.element_size() for w in self.weights for t in w[2:] if t.numel() > 1)

    def step(self, batch):
        for n, k, *w in self.weights:
            if (batch, k) not in self.x:
                self.x[(batch, k)] = torch.randn(batch, k, device=w[0].device, dtype=torch.bfloat16)
            self.call(self.x[(batch, k)], n, k, *w)


def graph_time(fn, stream, steps, warmup):
    with torch.cuda.stream(stream):
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
    for family in FAMILIES:
        layers = args.layers
        m = Linears(dev, layers, bench.LLAMA3_8B_UNMERGED, family)
        if m.bytes < COLD_BYTES:  # the small formats: as many more layers as put the weight set past twice the last-level cache
            layers *= -(-COLD_BYTES // m.bytes)
            del m
            m = Linears(dev, layers, bench.LLAMA3_8B_UNMERGED, family)
        sec = graph_time(lambda: m.step(1), stream, args.steps, args.warmup) * args.layers / layers  # per args.layers layers
        res[family] = {"tok_s": 1.0 / sec, "step_us": sec * 1e6, "layers": args.layers, "layers_measured": layers, "weight_bytes_measured": m.bytes,
                       "hbm_fraction": m.bytes * args.layers / layers / sec / HBM_BPS}
        del m
        torch.cuda.empty_cache()
    for name, d, _ in FORMATS:
        res[f"codebook_{name}_d{d}"]["vs_dequantize_linear"] = res[f"codebook_{name}_d{d}_dequantize_linear"]["step_us"] / res[f"codebook_{name}_d{d}"]["step_us"]
    return res


def gather(args, dev, emit):
    """What the LDS gather's bank conflicts cost at most: the fused linear at M = 1 with random codes next to the same launch with every
    code equal (all lanes read one address: a broadcast, no conflict), weights from HBM.  Replicating or skewing the table cannot win
    more than the difference."""
    n = kk = 4096
    x = torch.randn(1, kk, device=dev, dtype=torch.bfloat16)
    for name, d, k in FORMATS:
        copies = max(2, -(-COLD_BYTES // (n * kk // d // (2 if k == 16 else 1))))
        ws = [fields(torch.empty(n, kk, device=dev, dtype=torch.bfloat16), d, k) for _ in range(copies)]
        r = {"gather": f"{n}x{kk}", "codes": name, "d": d, "k": k, "copies": copies}
        r["random_codes_us"] = windows(lambda i: _fused(x, n, kk, *ws[i]), copies, max(args.reps, copies))
        for c, _, _ in ws:
            c.fill_(0x77)
        r["equal_codes_us"] = windows(lambda i: _fused(x, n, kk, *ws[i]), copies, max(args.reps, copies))
        r["conflict_share"] = 1.0 - min(r["equal_codes_us"]) / min(r["random_codes_us"])
        emit(r)
        del ws
        torch.cuda.empty_cache()


def sweep(args, dev, emit):
    for d, k in ((1, 256), (2, 256), (4, 256), (8, 256)):
        for name, n, kk in bench.LLAMA3_8B_UNMERGED:
            copies = max(2, -(-COLD_BYTES // (n * kk // d)))
            ws = [fields(torch.empty(n, kk, device=dev, dtype=torch.bfloat16), d, k) for _ in range(copies)]
            reps = max(args.reps, copies)
            for m in SWEEP_M:
                x = torch.randn(m, kk, device=dev, dtype=torch.bfloat16)
                r = {"sweep": name, "d": d, "k": k, "M": m, "N": n, "K": kk, "copies": copies, "reps": reps}
                r["fused_us"] = windows(lambda i: _fused(x, n, kk, *ws[i]), copies, reps)
                r["dequantize_linear_us"] = windows(lambda i: F.linear(x, ops.codebook_dequantize(*ws[i])), copies, reps)
                emit(r)
            del ws
            torch.cuda.empty_cache()


def fit(rows, emit):
    """Per format the seam s (fused up to s rows, dequantize + F.linear beyond) with the least time summed over the five shapes and every
    swept M (the fastest window of each cell); `spread_us`: the summed (max - min) of the windows, the margin of the fit."""
    for d in sorted({r["d"] for r in rows}):
        rs = [r for r in rows if r["d"] == d]
        ms = sorted({r["M"] for r in rs})
        total = {s: sum(min(r["fused_us"]) if r["M"] <= s else min(r["dequantize_linear_us"]) for r in rs) for s in [0] + ms}
        per_m = {str(m): [round(sum(min(r[key]) for r in rs if r["M"] == m), 1) for key in ("fused_us", "dequantize_linear_us")] for m in ms}
        spread = round(sum(max(r[key]) - min(r[key]) for r in rs for key in ("fused_us", "dequantize_linear_us")), 1)
        emit({"fit": "codebook", "d": d, "seam": min(total, key=total.get), "summed_us_by_seam": {str(s): round(v, 1) for s, v in total.items()},
              "five_shape_us_by_M_fused_vs_dequantize_linear": per_m, "spread_us": spread})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=bench.N_LAYERS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-lloyd", action="store_true")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_codebook.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)
        if out:
            out.write(json.dumps(r) + "\n")
            out.flush()

    with torch.no_grad():
        if not args.no_lloyd:
            lloyd(dev, emit)
            from_float(dev, emit)
        if not args.no_decode:
            emit({"decode_bs1_llama3_8b_five_shape": decode(args, dev)})
            gather(args, dev, emit)
        if args.sweep:
            sweep(args, dev, emit)
            fit([r for r in rows if "sweep" in r], emit)


if __name__ == "__main__":
    main()
