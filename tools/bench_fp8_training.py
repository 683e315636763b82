#!/usr/bin/env python3
"""float8 training in one process: the HIP training casts as HBM streams next to the same casts composed from eager
PyTorch ops, and forward + backward of Float8Linear per recipe next to bf16 nn.Linear autograd and MXFP8Linear.

  casts    [8192, 4096], [8192, 14336], [16384, 4096] bf16.  Every timed call takes the next of enough input buffers that together they are
           3 x the 256 MB last-level cache, so no call finds its input there.  Per shape, with round_scales_to_power_of_2:
             row_us       ops.fp8_train_quantize_rowwise (one launch)            5 bytes an element: read 2 for the amax, read 2, write 1
             col_t_us     ops.fp8_train_quantize_colwise_t (amax + cast)         5 bytes an element
             both_us      ops.fp8_train_quantize_both (amax + cast)              6 bytes an element: read 2, read 2, write 1 + 1
             two_call_us  the row call followed by the column call               (10 bytes an element moved; the same 6 are needed)
             eager_*_us   the same casts from eager ops: abs, amax, float64 division, mul, clamp, to(float8), and .t().contiguous()
           *_gbps: the algorithmic bytes over the time.  speedup_both_vs_two_call = two_call_us / both_us.
  linears  the five Llama-3-8B shapes (bench.py's LLAMA3_8B_UNMERGED) at M = 8192 tokens, bias-free, input and weight requiring grad.
           Per recipe (rowwise, rowwise_with_gw_hp, tensorwise_e4m3 = the default config with grad_output cast to e4m3):
           fwd_bwd_us, casts_us (the step's casts alone, called as the Function calls them), cast_share = casts_us / fwd_bwd_us,
           speedup_vs_bf16 = bf16_fwd_bwd_us / fwd_bwd_us; mxfp8_fwd_bwd_us of MXFP8Linear in the same process.
Device events around a window of calls, the median window of the replays, per call.
    python tools/bench_fp8_training.py [--replays 7] [--only casts|linears] [--out profiles/fp8_training.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ao_amd import ops  # noqa: E402
from ao_amd.float8 import CastConfig, Float8LinearConfig, e4m3_dtype  # noqa: E402
from ao_amd.float8 import float8_linear as FL  # noqa: E402
from ao_amd.prototype.mx_training import MXFP8Linear  # noqa: E402

CASTS = [(8192, 4096), (8192, 14336), (16384, 4096)]
M_TOKENS = 8192
LINEARS = {"qkv": (6144, 4096), "o": (4096, 4096), "gate": (14336, 4096), "up": (14336, 4096), "down": (4096, 14336)}
LLC_BYTES = 256 << 20
RECIPES = {
    "rowwise": lambda: Float8LinearConfig.from_recipe_name("rowwise"),
    "rowwise_with_gw_hp": lambda: Float8LinearConfig.from_recipe_name("rowwise_with_gw_hp"),
    "tensorwise_e4m3": lambda: Float8LinearConfig(cast_config_grad_output=CastConfig(target_dtype=e4m3_dtype)),
}


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


def _scale(amax, pow2):
    s = (448.0 / amax.to(torch.float64).clamp(min=1e-12)).to(torch.float32)
    return torch.exp2(torch.floor(torch.log2(s))) if pow2 else s


def eager_row(x, pow2=True):
    s = _scale(x.abs().amax(dim=1, keepdim=True), pow2)
    return (x.to(torch.float32) * s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn), s


def eager_col_t(x, pow2=True):
    s = _scale(x.abs().amax(dim=0, keepdim=True), pow2)
    return (x.to(torch.float32) * s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).t().contiguous(), s


def cast(r, c, dev, replays):
    nbuf = max(2, -(-3 * LLC_BYTES // (r * c * 2)))
    xs = [torch.randn(r, c, device=dev, dtype=torch.bfloat16) for _ in range(nbuf)]
    rec = {"kind": "cast", "R": r, "C": c, "buffers": nbuf, "replays": replays, "pow2": True}
    forms = {
        "row": lambda i: ops.fp8_train_quantize_rowwise(xs[i], True),
        "col_t": lambda i: ops.fp8_train_quantize_colwise_t(xs[i], True),
        "both": lambda i: ops.fp8_train_quantize_both(xs[i], True),
        "two_call": lambda i: (ops.fp8_train_quantize_rowwise(xs[i], True), ops.fp8_train_quantize_colwise_t(xs[i], True)),
        "amax_both": lambda i: ops.fp8_train_amax(xs[i], True, True),
        "eager_row": lambda i: eager_row(xs[i]),
        "eager_col_t": lambda i: eager_col_t(xs[i]),
        "eager_both": lambda i: (eager_row(xs[i]), eager_col_t(xs[i])),
    }
    bytes_per = {"row": 5, "col_t": 5, "both": 6, "two_call": 6, "amax_both": 2, "eager_row": 5, "eager_col_t": 5, "eager_both": 6}
    for name, fn in forms.items():
        us = window_us(fn, nbuf, replays)
        rec[name + "_us"] = us
        rec[name + "_gbps"] = r * c * bytes_per[name] / (us * 1e-6) / 1e9
    rec["speedup_both_vs_two_call"] = rec["two_call_us"] / rec["both_us"]
    rec["speedup_both_vs_eager"] = rec["eager_both_us"] / rec["both_us"]
    rec["speedup_row_vs_eager"] = rec["eager_row_us"] / rec["row_us"]
    rec["speedup_col_t_vs_eager"] = rec["eager_col_t_us"] / rec["col_t_us"]
    return rec


def step_casts(c, x, w, go):
    """The casts of one forward + backward under config c, called as matmul_with_hp_or_float8_args calls them."""
    p = c.round_scales_to_power_of_2
    if FL._gemm_is_fp8(c.cast_config_input, c.cast_config_weight):
        FL._cast(x, c.cast_config_input, None, p)
        FL._cast(w, c.cast_config_weight, None, p)
    gi = FL._gemm_is_fp8(c.cast_config_grad_output, c.cast_config_weight_for_grad_input)
    gw = FL._gemm_is_fp8(c.cast_config_grad_output_for_grad_weight, c.cast_config_input_for_grad_weight)
    if gi or gw:
        FL._cast(go, c.cast_config_grad_output if gi else None, c.cast_config_grad_output_for_grad_weight if gw else None, p)
    if gi:
        FL._cast(w, None, c.cast_config_weight_for_grad_input, p)
    if gw:
        FL._cast(x, None, c.cast_config_input_for_grad_weight, p)


def linear(name, dev, replays):
    n, k = LINEARS[name]
    m = M_TOKENS
    x = torch.randn(m, k, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    go = torch.randn(m, n, device=dev, dtype=torch.bfloat16) * 0.01
    ref = torch.nn.Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16)
    mxl = MXFP8Linear(k, n, bias=False, device=dev, dtype=torch.bfloat16)
    rec = {"kind": "linear", "cell": name, "M": m, "N": n, "K": k, "replays": replays}

    def step(mod):
        x.grad = mod.weight.grad = None
        mod(x).backward(go)

    rec["bf16_fwd_bwd_us"] = window_us(lambda i: step(ref), 1, replays)
    rec["mxfp8_fwd_bwd_us"] = window_us(lambda i: step(mxl), 1, replays)
    for tag, make in RECIPES.items():
        cfg = make()
        mod = FL.Float8Linear.from_float(ref, cfg)
        us = window_us(lambda i: step(mod), 1, replays)
        with torch.no_grad():
            casts = window_us(lambda i: step_casts(cfg, x, ref.weight, go), 1, replays)
        rec[tag] = {"fwd_bwd_us": us, "casts_us": casts, "cast_share": casts / us, "speedup_vs_bf16": rec["bf16_fwd_bwd_us"] / us,
                    "speedup_vs_mxfp8": rec["mxfp8_fwd_bwd_us"] / us}
    x.grad = ref.weight.grad = None
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
        sys.exit("bench_fp8_training.py measures on the GPU: no device visible")
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
