#!/usr/bin/env python3
"""NVFP4 training in one process: the casts as HBM streams against their algorithmic bytes, the fused row + column cast
next to a row-only plus a column-only call, and forward + backward of NVFP4Linear next to bf16 nn.Linear autograd, Float8Linear (rowwise)
and MXFP8Linear.

  casts    bf16 [M, N] of 16, 64, 224 and 512 MiB.  Every timed call takes the next of enough input buffers that together they are 3 x the
           256 MB last-level cache (at least two), so no call finds its input there.  Per shape and rounding (rtne, sr):
             amax_us       ops.nvfp4_train_amax (both amaxes)                              2 bytes an element
             fused_us      ops.nvfp4_train_quantize_row_col, both outputs                  2 + 2 x 0.5625 bytes an element
             row_us, col_us   one direction a call                                         2 + 0.5625 bytes an element
             two_call_us   the row call followed by the column call                        (the same 3.125 are needed; 5.125 are moved)
             weight_us     ops.nvfp4_train_quantize_weight_2d, both directions (rtne only) 2 + 2 x 0.5625 bytes an element
           *_gbps: the algorithmic bytes over the time.  fused_vs_two_call = two_call_us / fused_us: above 1 the fused call wins.
  linears  the five Llama-3-8B shapes at M = 8192 tokens, bias-free, input and weight requiring grad; a step's operands and outputs are
           beyond the last-level cache, so the weights come from HBM.  fwd_bwd_us of NVFP4Linear, its casts alone (casts_us, called as the
           Function calls them) and its three GEMMs alone (out_us, grad_input_us, grad_weight_us, each next to the bf16 matmul of the same
           shape), bf16 / rowwise / mxfp8 fwd_bwd_us in the same process, speedup_vs_* = that module's fwd_bwd_us / NVFP4Linear's.
           The GEMM-alone figures (and casts_us) replay ONE set of operands in windows of one call: at llama3_o operands and output (some 90 - 160 MiB)
           fit the last-level cache, so they are WARM figures, unlike the casts and the whole step; the GEMMs are compute-bound.
Device events around a window of calls, the median window of the replays, per call.
    python tools/bench_nvfp4_training.py [--replays 7] [--only casts|linears] [--out profiles/nvfp4_training.jsonl]"""
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
from ao_amd.prototype.mx_training import MXFP8Linear  # noqa: E402
from ao_amd.prototype.nvfp4_training import DEFAULT_SIGN_VECTOR, NVFP4Linear  # noqa: E402

CASTS = [(2048, 4096), (8192, 4096), (8192, 14336), (16384, 16384)]
M_TOKENS = 8192
LINEARS = {"llama3_qkv": (6144, 4096), "llama3_o": (4096, 4096), "llama3_gate": (14336, 4096), "llama3_up": (14336, 4096),
           "llama3_down": (4096, 14336)}
LLC_BYTES = 256 << 20
CODE_BYTES = 0.5625  # half a byte of codes and a sixteenth of a scale byte an element


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


def cast(m, n, dev, replays):
    nbuf = max(2, -(-3 * LLC_BYTES // (m * n * 2)))
    xs = [torch.randn(m, n, device=dev, dtype=torch.bfloat16) for _ in range(nbuf)]
    mask = ops.nvfp4_sign_mask(DEFAULT_SIGN_VECTOR)
    amax2 = ops.nvfp4_train_amax(xs[0], mask)
    seed = torch.tensor([1234567], dtype=torch.int64, device=dev)
    co, ro = torch.tensor([1], dtype=torch.int64, device=dev), torch.tensor([2], dtype=torch.int64, device=dev)
    rec = {"kind": "cast", "M": m, "N": n, "mib": m * n * 2 / 2 ** 20, "buffers": nbuf, "replays": replays}
    rec["amax_us"] = window_us(lambda i: ops.nvfp4_train_amax(xs[i], mask), nbuf, replays)
    rec["amax_gbps"] = m * n * 2 / (rec["amax_us"] * 1e-6) / 1e9
    rec["weight_us"] = window_us(lambda i: ops.nvfp4_train_quantize_weight_2d(xs[i], amax2[1]), nbuf, replays)
    rec["weight_gbps"] = m * n * (2 + 2 * CODE_BYTES) / (rec["weight_us"] * 1e-6) / 1e9
    for tag, sr in (("rtne", (None, None, None)), ("sr", (seed, co, ro))):
        def q(i, **kw):
            return ops.nvfp4_train_quantize_row_col(xs[i], amax2, mask, *sr, **kw)

        forms = {"fused": (2 + 2 * CODE_BYTES, lambda i: q(i)), "row": (2 + CODE_BYTES, lambda i: q(i, want_col=False)),
                 "col": (2 + CODE_BYTES, lambda i: q(i, want_row=False)),
                 "two_call": (2 + 2 * CODE_BYTES, lambda i: (q(i, want_col=False), q(i, want_row=False)))}
        for name, (bytes_per, fn) in forms.items():
            us = window_us(fn, nbuf, replays)
            rec[f"{tag}_{name}_us"] = us
            rec[f"{tag}_{name}_gbps"] = m * n * bytes_per / (us * 1e-6) / 1e9
        rec[f"{tag}_fused_vs_two_call"] = rec[f"{tag}_two_call_us"] / rec[f"{tag}_fused_us"]
    return rec


def linear(name, dev, replays):
    n, k = LINEARS[name]
    m = M_TOKENS
    x = torch.randn(m, k, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    go = torch.randn(m, n, device=dev, dtype=torch.bfloat16) * 0.01
    ref = torch.nn.Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16)
    mx = MXFP8Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16)
    mods = {"nvfp4": NVFP4Linear.from_linear(ref, rht_sign_vector=DEFAULT_SIGN_VECTOR), "bf16": ref,
            "rowwise": Float8Linear.from_float(ref, Float8LinearConfig.from_recipe_name("rowwise")), "mxfp8": mx}
    rec = {"kind": "linear", "cell": name, "M": m, "N": n, "K": k, "replays": replays}

    def step(mod):
        x.grad = mod.weight.grad = None
        mod(x).backward(go)

    for tag, mod in mods.items():
        rec[tag + "_fwd_bwd_us"] = window_us(lambda i: step(mod), 1, replays)
    x.grad = ref.weight.grad = mx.weight.grad = None
    xd, w = x.detach(), ref.weight.detach()
    mask = ops.nvfp4_sign_mask(DEFAULT_SIGN_VECTOR)
    seed = torch.tensor([1234567], dtype=torch.int64, device=dev)
    co, ro = torch.tensor([1], dtype=torch.int64, device=dev), torch.tensor([2], dtype=torch.int64, device=dev)

    def casts():
        xa = ops.nvfp4_train_amax(xd, mask)
        ops.nvfp4_train_quantize_row_col(xd, xa, mask)
        ops.nvfp4_train_quantize_weight_2d(w, ops.nvfp4_train_amax(w, 0, want_rht=False)[1])
        ga = ops.nvfp4_train_amax(go, mask)
        ops.nvfp4_train_quantize_row_col(go, ga, mask, seed, co, ro)

    rec["casts_us"] = window_us(lambda i: casts(), 1, replays)
    xa, wa, ga = ops.nvfp4_train_amax(xd, mask), ops.nvfp4_train_amax(w, 0, want_rht=False)[1], ops.nvfp4_train_amax(go, mask)
    xcq, xcs, xrq, xrs = ops.nvfp4_train_quantize_row_col(xd, xa, mask)
    wq, ws, wtq, wts = ops.nvfp4_train_quantize_weight_2d(w, wa)
    gcq, gcs, grq, grs = ops.nvfp4_train_quantize_row_col(go, ga, mask, seed, co, ro)
    one = torch.ones((), dtype=torch.float32, device=dev)
    rec["out_us"] = window_us(lambda i: ops.nvfp4_scaled_mm(xrq, xrs, wq, ws, one, one), 1, replays)
    rec["grad_input_us"] = window_us(lambda i: ops.nvfp4_scaled_mm(grq, grs, wtq, wts, one, one), 1, replays)
    rec["grad_weight_us"] = window_us(lambda i: ops.nvfp4_scaled_mm(gcq, gcs, xcq, xcs, one, one), 1, replays)
    rec["bf16_out_us"] = window_us(lambda i: torch.mm(xd, w.t()), 1, replays)
    rec["bf16_grad_input_us"] = window_us(lambda i: torch.mm(go, w), 1, replays)
    rec["bf16_grad_weight_us"] = window_us(lambda i: torch.mm(go.t(), xd), 1, replays)
    for tag in ("out", "grad_input", "grad_weight"):
        rec[tag + "_tflops"] = 2.0 * m * n * k / (rec[tag + "_us"] * 1e-6) / 1e12
    rec["cast_share"] = rec["casts_us"] / rec["nvfp4_fwd_bwd_us"]
    for tag in ("bf16", "rowwise", "mxfp8"):
        rec["speedup_vs_" + tag] = rec[tag + "_fwd_bwd_us"] / rec["nvfp4_fwd_bwd_us"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=7, help="timed windows per figure (the median is recorded; at least 5)")
    ap.add_argument("--only", choices=["casts", "linears"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.replays < 5:
        ap.error("--replays must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_nvfp4_training.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None
    jobs = []
    if args.only in (None, "casts"):
        jobs += [lambda m=m, n=n: cast(m, n, dev, args.replays) for m, n in CASTS]
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
