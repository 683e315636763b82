#!/usr/bin/env python3
"""Blockwise float8 training in one process: the block-local casts as HBM streams next to the rowwise training casts,
the weight-gradient GEMM next to the MXFP8 one, and forward + backward of Float8BlockwiseLinear next to bf16 nn.Linear autograd,
Float8Linear (rowwise) and MXFP8Linear.

  casts    [8192, 4096], [8192, 14336], [16384, 4096] bf16.  Every timed call takes the next of enough input buffers that together they are
           3 x the 256 MB last-level cache, so no call finds its input there.  Per shape:
             rows_us      ops.fp8_block_train_cast(x, rows=True)                 3 bytes an element: read 2, write 1
             cols_us      ops.fp8_block_train_cast(x, rows=False, cols=True)     3 bytes an element
             both_us      ops.fp8_block_train_cast(x, rows=True, cols=True)      4 bytes an element: read 2, write 1 + 1
             two_call_us  the rows call followed by the columns call             (6 bytes an element moved; the same 4 are needed)
             weight_us, weight_t_us   ops.fp8_block_train_cast_weight, plain and transposed    3 bytes an element
             rowwise_us, colwise_t_us ops.fp8_train_quantize_rowwise / _colwise_t, which read x twice: 5 bytes an element
           *_gbps: the algorithmic bytes over the time.
  wgrads   the linears' shapes: ops.fp8_block_mm_wgrad next to ops.mxfp8_mm_wgrad on casts of the same tensors (the same staging, the same
           MFMA); *_tflops = 2 M N K over the time.
  linears  the five Llama-3-8B shapes and DeepSeek-V3's dense shapes at M = 8192 tokens, bias-free, input and weight requiring grad:
           fwd_bwd_us of Float8BlockwiseLinear, its casts alone (casts_us, called as the Function calls them) and its three GEMMs alone
           (out_us, grad_input_us, grad_weight_us, each next to the bf16 matmul of the same shape), cast_share = casts_us / fwd_bwd_us,
           bf16 / rowwise / mxfp8 fwd_bwd_us in the same process, speedup_vs_bf16 = bf16_fwd_bwd_us / fwd_bwd_us.
Device events around a window of calls, the median window of the replays, per call.
    python tools/bench_fp8_block_training.py [--replays 7] [--only casts|wgrads|linears] [--out profiles/fp8_block_training.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ao_amd import ops  # noqa: E402
from ao_amd.float8 import Float8LinearConfig  # noqa: E402
from ao_amd.float8.float8_linear import Float8Linear  # noqa: E402
from ao_amd.prototype.blockwise_fp8_training import Float8BlockwiseLinear  # noqa: E402
from ao_amd.prototype.mx_training import MXFP8Linear  # noqa: E402

CASTS = [(8192, 4096), (8192, 14336), (16384, 4096)]
M_TOKENS = 8192
LINEARS = {"llama3_qkv": (6144, 4096), "llama3_o": (4096, 4096), "llama3_gate": (14336, 4096), "llama3_up": (14336, 4096),
           "llama3_down": (4096, 14336), "deepseek_v3_proj": (7168, 2048), "deepseek_v3_down": (7168, 18432),
           "deepseek_v3_up": (18432, 7168), "deepseek_v3_q_a": (1536, 7168)}
LLC_BYTES = 256 << 20


def window_us(fn, calls, replays):
    """Median over `replays` windows of `calls` calls fn(i), per call; one untimed window first."""
    for i in range(calls):
        fn(i)
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / calls)
    return statistics.median(times)


def cast(r, c, dev, replays):
    nbuf = max(2, -(-3 * LLC_BYTES // (r * c * 2)))
    xs = [torch.randn(r, c, device=dev, dtype=torch.bfloat16) for _ in range(nbuf)]
    rec = {"kind": "cast", "R": r, "C": c, "buffers": nbuf, "replays": replays}
    forms = {
        "rows": (3, lambda i: ops.fp8_block_train_cast(xs[i], rows=True, cols=False)),
        "cols": (3, lambda i: ops.fp8_block_train_cast(xs[i], rows=False, cols=True)),
        "both": (4, lambda i: ops.fp8_block_train_cast(xs[i], rows=True, cols=True)),
        "two_call": (4, lambda i: (ops.fp8_block_train_cast(xs[i], rows=True, cols=False), ops.fp8_block_train_cast(xs[i], rows=False, cols=True))),
        "weight": (3, lambda i: ops.fp8_block_train_cast_weight(xs[i], transposed=False)),
        "weight_t": (3, lambda i: ops.fp8_block_train_cast_weight(xs[i], transposed=True)),
        "rowwise": (5, lambda i: ops.fp8_train_quantize_rowwise(xs[i], False)),
        "colwise_t": (5, lambda i: ops.fp8_train_quantize_colwise_t(xs[i], False)),
    }
    for name, (bytes_per, fn) in forms.items():
        us = window_us(fn, nbuf, replays)
        rec[name + "_us"] = us
        rec[name + "_gbps"] = r * c * bytes_per / (us * 1e-6) / 1e9
    rec["speedup_both_vs_two_call"] = rec["two_call_us"] / rec["both_us"]
    rec["rows_vs_rowwise"] = rec["rowwise_us"] / rec["rows_us"]
    rec["cols_vs_colwise_t"] = rec["colwise_t_us"] / rec["cols_us"]
    return rec


def wgrad(name, dev, replays):
    n, k = LINEARS[name]
    m = M_TOKENS
    x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
    go = torch.randn(m, n, device=dev, dtype=torch.bfloat16) * 0.01
    _, (g_t, g_inv) = ops.fp8_block_train_cast(go, rows=False, cols=True)
    _, (x_t, x_inv) = ops.fp8_block_train_cast(x, rows=False, cols=True)
    mg_t, mg_s = ops.mxfp8_quantize_colwise(go, "rceil")
    mx_t, mx_s = ops.mxfp8_quantize_colwise(x, "rceil")
    rec = {"kind": "wgrad", "cell": name, "M": m, "N": n, "K": k, "replays": replays}
    rec["block_us"] = window_us(lambda i: ops.fp8_block_mm_wgrad(g_t, g_inv, x_t, x_inv), 1, replays)
    rec["mxfp8_us"] = window_us(lambda i: ops.mxfp8_mm_wgrad(mg_t, mg_s, mx_t, mx_s, n, k), 1, replays)
    rec["bf16_us"] = window_us(lambda i: torch.mm(go.t(), x), 1, replays)
    for tag in ("block", "mxfp8", "bf16"):
        rec[tag + "_tflops"] = 2.0 * m * n * k / (rec[tag + "_us"] * 1e-6) / 1e12
    rec["block_vs_mxfp8"] = rec["mxfp8_us"] / rec["block_us"]
    return rec


def linear(name, dev, replays):
    n, k = LINEARS[name]
    m = M_TOKENS
    x = torch.randn(m, k, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    go = torch.randn(m, n, device=dev, dtype=torch.bfloat16) * 0.01
    ref = torch.nn.Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16)
    mods = {"bf16": ref, "block": Float8BlockwiseLinear.from_float(ref),
            "rowwise": Float8Linear.from_float(ref, Float8LinearConfig.from_recipe_name("rowwise")),
            "mxfp8": MXFP8Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16)}
    rec = {"kind": "linear", "cell": name, "M": m, "N": n, "K": k, "replays": replays}

    def step(mod):
        x.grad = mod.weight.grad = None
        mod(x).backward(go)

    for tag, mod in mods.items():
        rec[tag + "_fwd_bwd_us"] = window_us(lambda i: step(mod), 1, replays)
    x.grad = ref.weight.grad = None
    xd, w = x.detach(), ref.weight.detach()

    def casts():
        ops.fp8_block_train_cast(xd, rows=True, cols=False)
        ops.fp8_block_train_cast_weight(w, transposed=False)
        ops.fp8_block_train_cast(go, rows=True, cols=True)
        ops.fp8_block_train_cast_weight(w, transposed=True)
        ops.fp8_block_train_cast(xd, rows=False, cols=True)

    rec["casts_us"] = window_us(lambda i: casts(), 1, replays)
    (xq, xi), (xt, xti) = ops.fp8_block_train_cast(xd, rows=True, cols=True)
    (wq, wi), (wt, wti) = ops.fp8_block_train_cast_weight(w, transposed=None)
    (gq, gi), (gt, gti) = ops.fp8_block_train_cast(go, rows=True, cols=True)
    rec["out_us"] = window_us(lambda i: ops.fp8_block_mm(xq, xi, wq, wi), 1, replays)
    rec["grad_input_us"] = window_us(lambda i: ops.fp8_block_mm(gq, gi, wt, wti), 1, replays)
    rec["grad_weight_us"] = window_us(lambda i: ops.fp8_block_mm_wgrad(gt, gti, xt, xti), 1, replays)
    rec["bf16_out_us"] = window_us(lambda i: torch.mm(xd, w.t()), 1, replays)
    rec["bf16_grad_input_us"] = window_us(lambda i: torch.mm(go, w), 1, replays)
    rec["bf16_grad_weight_us"] = window_us(lambda i: torch.mm(go.t(), xd), 1, replays)
    rec["cast_share"] = rec["casts_us"] / rec["block_fwd_bwd_us"]
    for tag in ("bf16", "rowwise", "mxfp8"):
        rec["speedup_vs_" + tag] = rec[tag + "_fwd_bwd_us"] / rec["block_fwd_bwd_us"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=7, help="timed windows per figure (the median is recorded; at least 5)")
    ap.add_argument("--only", choices=["casts", "wgrads", "linears"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.replays < 5:
        ap.error("--replays must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_fp8_block_training.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None
    jobs = []
    if args.only in (None, "casts"):
        jobs += [lambda r=r, c=c: cast(r, c, dev, args.replays) for r, c in CASTS]
    if args.only in (None, "wgrads"):
        jobs += [lambda name=name: wgrad(name, dev, args.replays) for name in LINEARS]
    if args.only in (None, "linears"):
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
