#!/usr/bin/env python3
"""MXFP8 dense-linear training in one process: the one-pass rowwise + colwise cast next to the two launches it replaces,
and forward + backward of MXFP8Linear next to bf16 nn.Linear autograd.

  casts    [8192, 4096], [8192, 14336], [16384, 6144] bf16 (64 MiB to 224 MiB read: at or beyond the last-level cache together with the
           outputs).  Per shape: rowcol_us (ops.mxfp8_quantize_rowcol), rowwise_us + colwise_us (ops.mxfp8_quantize, ops.mxfp8_quantize_colwise),
           the achieved TB/s of each side (4.0625 bytes an element against 6.0625: x read once against twice) and speedup = two / one.
  linears  the five Llama-3-8B shapes (bench.py's LLAMA3_8B_UNMERGED) at M = 8192 tokens: W [N, K] = qkv [6144, 4096], o [4096, 4096],
           gate and up [14336, 4096], down [4096, 14336].
           fwd_bwd_us of MXFP8Linear and bf16_fwd_bwd_us of nn.Linear (both bias-free, input and weight requiring grad), speedup = bf16 / mxfp8;
           each launch of the backward alone: cast_go_us (the cast of grad_out the Function takes), cast_w_colwise_us + w_scale_t_us (the
           weight along N and the copy that brings its scales to [K][N/32]), dgrad_us (ops.mx_mm), cast_x_colwise_us, wgrad_us
           (ops.mxfp8_mm_wgrad); wgrad_fp8_peak_fraction = 2 M N K / wgrad_us over the dense fp8 MFMA peak (ao_amd/roofline.py).
Eager calls between two events, the median of the replays.
    python tools/bench_mxfp8_linear_bwd.py [--replays 7] [--only casts|linears] [--one-pass | --two-launches] [--out profiles/mxfp8_linear_bwd.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ao_amd import ops, roofline  # noqa: E402
from ao_amd.prototype import mx  # noqa: E402
from ao_amd.prototype.mx_training import MXFP8Linear  # noqa: E402

CASTS = [(8192, 4096), (8192, 14336), (16384, 6144)]
M_TOKENS = 8192
LINEARS = {"qkv": (6144, 4096), "o": (4096, 4096), "gate": (14336, 4096), "up": (14336, 4096), "down": (4096, 14336)}


def eager_us(fn, replays):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times)


def cast(r, c, dev, replays):
    x = torch.randn(r, c, device=dev, dtype=torch.bfloat16)
    rec = {"kind": "cast", "R": r, "C": c, "replays": replays}
    rec["rowcol_us"] = eager_us(lambda: ops.mxfp8_quantize_rowcol(x), replays)
    rec["rowwise_us"] = eager_us(lambda: ops.mxfp8_quantize(x), replays)
    rec["colwise_us"] = eager_us(lambda: ops.mxfp8_quantize_colwise(x), replays)
    rec["two_launches_us"] = eager_us(lambda: (ops.mxfp8_quantize(x), ops.mxfp8_quantize_colwise(x)), replays)
    rec["rowcol_tbps"] = r * c * 4.0625 / (rec["rowcol_us"] * 1e-6) / 1e12
    rec["two_launches_tbps"] = r * c * 6.0625 / (rec["two_launches_us"] * 1e-6) / 1e12
    rec["speedup"] = rec["two_launches_us"] / rec["rowcol_us"]
    return rec


def linear(name, dev, replays):
    n, k = LINEARS[name]
    m = M_TOKENS
    x = torch.randn(m, k, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    go = torch.randn(m, n, device=dev, dtype=torch.bfloat16) * 0.01
    mxl = MXFP8Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16)
    ref = torch.nn.Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16)
    rec = {"kind": "linear", "cell": name, "M": m, "N": n, "K": k, "replays": replays,
           "cast_go": {None: "by size", True: "one pass", False: "two launches"}[mx.ONE_PASS_CAST]}

    def step(mod):
        x.grad = mod.weight.grad = None
        mod(x).backward(go)

    rec["fwd_bwd_us"] = eager_us(lambda: step(mxl), replays)
    rec["bf16_fwd_bwd_us"] = eager_us(lambda: step(ref), replays)
    rec["speedup_vs_bf16"] = rec["bf16_fwd_bwd_us"] / rec["fwd_bwd_us"]
    x.grad = mxl.weight.grad = ref.weight.grad = None
    w = mxl.weight
    with torch.no_grad():
        rec["fwd_us"] = eager_us(lambda: mxl(x), replays)
        rec["bf16_fwd_us"] = eager_us(lambda: ref(x), replays)
        rec["cast_go_us"] = eager_us(lambda: mx.mxfp8_cast_both(go, "rceil"), replays)
        rec["cast_w_colwise_us"] = eager_us(lambda: ops.mxfp8_quantize_colwise(w), replays)
        go_q, go_s, go_t, go_ts = mx.mxfp8_cast_both(go, "rceil")
        w_t, w_ts = ops.mxfp8_quantize_colwise(w)
        rec["w_scale_t_us"] = eager_us(lambda: w_ts.contiguous(), replays)
        w_tc, w_tsc = w_t.t(), w_ts.contiguous()
        rec["dgrad_us"] = eager_us(lambda: ops.mx_mm(go_q, go_s, w_tc, w_tsc, None, ops.MX_FMT_E4M3), replays)
        del go_q, go_s, w_t, w_ts, w_tc, w_tsc
        rec["cast_x_colwise_us"] = eager_us(lambda: ops.mxfp8_quantize_colwise(x), replays)
        x_t, x_ts = ops.mxfp8_quantize_colwise(x)
        rec["wgrad_us"] = eager_us(lambda: ops.mxfp8_mm_wgrad(go_t, go_ts, x_t, x_ts, n, k), replays)
    rec["wgrad_fp8_peak_fraction"] = 2.0 * m * n * k / (rec["wgrad_us"] * 1e-6) / roofline.get_specs()["fp8_peak_tops"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=7, help="timed calls per figure (the median is recorded; at least 5)")
    ap.add_argument("--only", choices=["casts", "linears"], default=None)
    ap.add_argument("--two-launches", action="store_true", help="the Functions cast grad_out by two launches (mx.ONE_PASS_CAST = False)")
    ap.add_argument("--one-pass", action="store_true", help="... by the one-pass kernel whatever the size (mx.ONE_PASS_CAST = True)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.replays < 5:
        ap.error("--replays must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_mxfp8_linear_bwd.py measures on the GPU: no device visible")
    if args.two_launches or args.one_pass:
        mx.ONE_PASS_CAST = bool(args.one_pass)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None
    jobs = []
    if args.only != "linears":
        jobs += [lambda r=r, c=c: cast(r, c, dev, args.replays) for r, c in CASTS]
    if args.only != "casts":
        jobs += [lambda name=name: linear(name, dev, args.replays) for name in LINEARS]
    for job in jobs:
        rec = json.dumps(job())
        print(rec, flush=True)
        if out:
            out.write(rec + "\n")
            out.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
