#!/usr/bin/env python3
"""The NF4 (QLoRA) kernels measured, everything in this one process:
  * streams: the cast (nf4_block_absmax + torch's mean + nf4_quantize) and nf4_dequantize as HBM streams over their algorithmic bytes
    (cast: 2 B read + 0.516 B written a weight; dequantize: 0.516 B read + 2 B written), next to the same chains written in eager PyTorch
    ops (the reference's op sequence: a [chunk, 16] broadcast subtract for the codes, a dozen ops for the dequantize);
  * decode: one token (bs = 1) through the Llama-3-8B five-shape x 32-layer linears, cold weights (bench.py's model: every layer its own
    weights), hipGraph replay: the fused NF4 linear, dequantize + F.linear, int4 (tinygemm layout, group 128), the NVFP4 weight-only
    linear and PyTorch's bf16 F.linear; tok/s and the weight bytes per second as a fraction of 8 TB/s;
  * --sweep: M = 1 .. 256 on the five shapes, us per linear for the fused form (forced) and for dequantize + F.linear, the weights rotated
    through enough copies that they come from HBM, each cell in WINDOWS repeated windows (their spread is the margin of the fit), then
    the `fit` line: the summed time per candidate seam;
  * --fit FILE: the seam a sweep file gives (no GPU);
  * --train: linear_nf4 forward + backward at M = 8192 next to a bf16 nn.Linear with a frozen weight and next to the eager dequantize chain.
    python tools/bench_nf4_linear.py [--steps 20] [--sweep] [--train] [--out profiles/nf4_linear.jsonl]"""
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
from ao_amd.quantization import linear_nf4, to_nf4  # noqa: E402
from ao_amd.quantization.nf4_tensor import NF4_TABLE  # noqa: E402

HBM_BPS = 8.0e12  # MI355X HBM3E peak
SWEEP_M = (1, 2, 4, 8, 16, 17, 24, 32, 33, 48, 64, 65, 96, 128, 192, 256)
COLD_BYTES = 512 << 20  # rotate a sweep's weight through copies worth this much: twice the last-level cache
WINDOWS = 3
B, SB = 64, 256
CHUNK = 1024 ** 2


# ---- the reference's chains in eager PyTorch ops (nf4_tensor.py:721-871), for the comparison only ------------------------------------------
def eager_cast(w, table):
    flat = w.flatten()
    blocks = flat.view(-1, B)
    a = blocks.abs().max(dim=1).values
    mean = a.mean()
    c = (a - mean).view(-1, SB)
    m = c.abs().max(dim=1).values.unsqueeze(-1)
    qf = 256 / (2 * m)
    q = (c * qf).round().clamp(-128, 127).flatten().to(torch.int8)
    v = (blocks / a.unsqueeze(-1)).flatten()
    codes = torch.empty(flat.numel(), dtype=torch.uint8, device=w.device)
    for s in range(0, flat.numel(), CHUNK):
        codes[s:s + CHUNK] = (v[s:s + CHUNK].unsqueeze(-1) - table).abs().min(dim=-1).indices.to(torch.uint8)
    return (codes[::2] << 4 | codes[1::2]), q, qf[:, 0].contiguous(), mean


def eager_dequantize(codes, q, qf, mean, table, shape):
    first, second = table[(codes >> 4).long()], table[(codes & 15).long()]
    s = (q.view(-1, SB) / qf.unsqueeze(-1)).flatten().to(torch.bfloat16) + mean
    rep = s.unsqueeze(-1).expand(s.size(0), B // 2).flatten()
    return torch.stack([first * rep, second * rep], dim=-1).reshape(shape)


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


def streams(args, dev, emit):
    table = torch.tensor(NF4_TABLE, dtype=torch.bfloat16, device=dev)
    for n, k in ((4096, 4096), (14336, 4096), (4096, 14336)):
        numel = n * k
        copies = max(2, -(-COLD_BYTES // (numel * 2)))
        ws = [torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(copies)]
        ts = [to_nf4(w, B, SB) for w in ws[:max(2, copies // 4)]]
        fields = lambda t: (t.quantized_data, t.quantized_scalers, t.quantization_factor, t.scaler_mean)  # noqa: E731
        cast_bytes = numel * 2 + numel // 2 + numel // B + 2 * numel // (B * SB)
        deq_bytes = numel // 2 + numel // B + 2 * numel // (B * SB) + numel * 2
        r = {"stream": f"{n}x{k}", "copies": copies}
        us = min(windows(lambda i: to_nf4(ws[i], B, SB), copies, 2 * copies))
        r["cast_us"], r["cast_GBps"] = us, cast_bytes / us / 1e3
        us = min(windows(lambda i: ops.nf4_dequantize(*fields(ts[i % len(ts)]), B, SB), len(ts), 4 * len(ts)))
        r["dequantize_us"], r["dequantize_GBps"] = us, deq_bytes / us / 1e3
        us = min(time_us(lambda i: eager_cast(ws[i], table), 2, 4) for _ in range(2))
        r["eager_cast_us"], r["eager_cast_GBps"] = us, cast_bytes / us / 1e3
        us = min(windows(lambda i: eager_dequantize(*fields(ts[i % len(ts)]), table, (n, k)), len(ts), 2 * len(ts)))
        r["eager_dequantize_us"], r["eager_dequantize_GBps"] = us, deq_bytes / us / 1e3
        r["cast_ahead"], r["dequantize_ahead"] = r["cast_us"] < r["eager_cast_us"], r["dequantize_us"] < r["eager_dequantize_us"]
        emit(r)
        del ws, ts
        torch.cuda.empty_cache()


# ---- decode -------------------------------------------------------------------------------------------------------------------------------------
def nf4_fields(w):
    t = to_nf4(w, B, SB)
    return t.quantized_data, t.quantized_scalers, t.quantization_factor, t.scaler_mean


def nvfp4_weight(w):
    p = ops.nvfp4_amax_scale(w)
    q, s = ops.nvfp4_quantize(w, p)
    return q, s, p


def _nf4_fused(x, n, k, *f):
    ops.nf4_set_form(1)
    try:
        return ops.nf4_linear(x, *f, n, k, B, SB)
    finally:
        ops.nf4_set_form(0)


FAMILIES = {
    # name: (prepare, call(x, n, k, *weight))
    "nf4": (nf4_fields, _nf4_fused),
    "nf4_dequantize_linear": (nf4_fields, lambda x, n, k, *f: F.linear(x, ops.nf4_dequantize(*f, B, SB).view(n, k))),
    "int4": (lambda w: ops.int4_quantize_tinygemm(w, 128), lambda x, n, k, q, sz: ops.weight_int4pack_mm(x, q, 128, sz)),
    "nvfp4_wo": (nvfp4_weight, lambda x, n, k, q, s, p: ops.nvfp4_wo_linear(x, q, s, p)),
    "bf16": (lambda w: (w,), lambda x, n, k, w: F.linear(x, w)),
}


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
    for other in ("nf4_dequantize_linear", "bf16", "int4", "nvfp4_wo"):
        res["nf4"]["vs_" + other] = res["nf4"]["tok_s"] / res[other]["tok_s"]
    res["route_bs1"] = {name: ops.nf4_linear_route(1, n, k, B, SB) for name, n, k in bench.LLAMA3_8B_UNMERGED}
    return res


# ---- the seam ---------------------------------------------------------------------------------------------------------------------------------
def sweep(args, dev, emit):
    for name, n, k in bench.LLAMA3_8B_UNMERGED:
        copies = max(2, -(-COLD_BYTES // (n * k * 33 // 64)))
        ws = []
        for _ in range(copies):
            w = torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.02
            ws.append(nf4_fields(w))
            del w
        reps = max(args.reps, 2 * copies)
        for m in SWEEP_M:
            x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
            r = {"sweep": name, "M": m, "N": n, "K": k, "copies": copies, "reps": reps, "route": ops.nf4_linear_route(m, n, k, B, SB)["kernel"]}
            ops.nf4_set_form(1)
            try:
                r["fused_us"] = windows(lambda i: ops.nf4_linear(x, *ws[i], n, k, B, SB), copies, reps)
            finally:
                ops.nf4_set_form(0)
            r["dequantize_linear_us"] = windows(lambda i: F.linear(x, ops.nf4_dequantize(*ws[i], B, SB).view(n, k)), copies, reps)
            emit(r)
        del ws
        torch.cuda.empty_cache()


def fit(path, emit=print):
    """The seam s (fused up to s rows, dequantize + F.linear beyond) with the least time summed over the five shapes and every swept M
    (the fastest window of each cell), per candidate the sum; `spread_us`: the summed (max - min) of the windows, the margin of the fit."""
    rows = [r for r in (json.loads(l) for l in open(path) if l.strip()) if "sweep" in r]
    if not rows:
        return
    ms = sorted({r["M"] for r in rows})
    total = {}
    for seam in [0] + ms:
        total[seam] = sum(min(r["fused_us"]) if r["M"] <= seam else min(r["dequantize_linear_us"]) for r in rows)
    per_m = {str(m): [round(sum(min(r["fused_us"]) for r in rows if r["M"] == m), 1),
                      round(sum(min(r["dequantize_linear_us"]) for r in rows if r["M"] == m), 1)] for m in ms}
    spread = {str(m): round(sum(max(r[key]) - min(r[key]) for r in rows if r["M"] == m for key in ("fused_us", "dequantize_linear_us")), 1)
              for m in ms}
    line = {"fit": "nf4", "seam": min(total, key=total.get), "summed_us_by_seam": {str(k): round(v, 1) for k, v in total.items()},
            "five_shape_us_by_M_fused_vs_dequantize_linear": per_m, "spread_us_by_M": spread}
    emit(line)


# ---- training rows -------------------------------------------------------------------------------------------------------------------------------
def train(args, dev, emit):
    table = torch.tensor(NF4_TABLE, dtype=torch.bfloat16, device=dev)
    M = 8192
    for n, k in ((4096, 4096), (14336, 4096)):
        w = torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.02
        t = to_nf4(w, B, SB)
        f = (t.quantized_data, t.quantized_scalers, t.quantization_factor, t.scaler_mean)
        x = torch.randn(M, k, device=dev, dtype=torch.bfloat16, requires_grad=True)
        go = torch.randn(M, n, device=dev, dtype=torch.bfloat16)
        lin = torch.nn.Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16)
        lin.weight.requires_grad_(False)

        def step(fwd):
            x.grad = None
            fwd().backward(go)

        def eager():
            eager_dequantize(*f, table, (n, k))  # (the reference dequantizes in the forward and again in the backward: two chains a step)
            return F.linear(x, eager_dequantize(*f, table, (n, k)))

        r = {"train": f"{M}x{n}x{k}"}
        for name, fwd in (("linear_nf4", lambda: linear_nf4(x, t)), ("bf16_frozen", lambda: lin(x)), ("eager_dequantize_chain", eager)):
            r[name + "_us"] = min(windows(lambda i: step(fwd), 2, 10))
        r["vs_bf16"], r["vs_eager_chain"] = r["bf16_frozen_us"] / r["linear_nf4_us"], r["eager_dequantize_chain_us"] / r["linear_nf4_us"]
        emit(r)
        del w, t, x, go, lin
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=bench.N_LAYERS)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--no-streams", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fit", default=None, metavar="JSONL", help="no GPU: print the fitted seam of a sweep file")
    args = ap.parse_args()
    if args.fit:
        return fit(args.fit, lambda r: print(json.dumps(r)))
    if not torch.cuda.is_available():
        sys.exit("bench_nf4_linear.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None

    def emit(r):
        print(json.dumps(r), flush=True)
        if out:
            out.write(json.dumps(r) + "\n")
            out.flush()

    with torch.no_grad():
        if not args.no_streams:
            streams(args, dev, emit)
        if not args.no_decode:
            emit({"decode_bs1_llama3_8b_five_shape": decode(args, dev)})
        if args.sweep:
            sweep(args, dev, emit)
            if args.out:
                fit(args.out, emit)
    if args.train:
        train(args, dev, emit)


if __name__ == "__main__":
    main()
