#!/usr/bin/env python3
"""Forward + backward of the MXFP8 MoE grouped GEMM next to bf16 autograd of torch._grouped_mm, in one process:

    cell               E    W [N, K]         tokens per expert
    mixtral_w1         8    [14336, 4096]    2048
    deepseek_v3_ep8    32   [2048, 7168]     2048   (one EP-8 rank's routed experts)

Per cell (eager calls between two events, the median of the replays; the weights alone are several times the last-level cache, so every
pass streams them cold from HBM):
  * fwd_bwd_us: _to_mxfp8_then_scaled_grouped_mm on tensors that require grad, then out.backward(grad_out);
  * each launch of the backward alone: cast_go_rowwise_us, cast_w_along_n_us, dgrad_us (ops.mxfp8_grouped_mm contracting over N),
    cast_go_colwise_us, cast_a_colwise_us, wgrad_us (ops.mxfp8_grouped_mm_wgrad); wgrad_fp8_peak_fraction = 2 M N K / wgrad_us over the
    dense fp8 MFMA peak (ao_amd/roofline.py);
  * bf16_fwd_bwd_us: torch._grouped_mm on the same bf16 tensors, forward and backward through autograd; speedup = bf16 / mxfp8.
    python tools/bench_mxfp8_grouped_bwd.py [--replays 7] [--cells mixtral_w1,deepseek_v3_ep8] [--out profiles/mxfp8_grouped_bwd.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ao_amd import ops, roofline  # noqa: E402
from ao_amd.prototype.mx import _to_mxfp8_then_scaled_grouped_mm  # noqa: E402

CELLS = {"mixtral_w1": (8, 14336, 4096, 2048), "deepseek_v3_ep8": (32, 2048, 7168, 2048)}


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


def cell(name, dev, replays):
    e, n, k, per = CELLS[name]
    m = e * per
    a = torch.randn(m, k, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    w = (torch.randn(e, n, k, device=dev, dtype=torch.bfloat16) * 0.02).requires_grad_(True)
    go = torch.randn(m, n, device=dev, dtype=torch.bfloat16) * 0.01
    offs = (torch.arange(1, e + 1) * per).to(torch.int32).to(dev)
    r = {"cell": name, "E": e, "N": n, "K": k, "M_total": m, "replays": replays}

    def step(mm):
        a.grad = w.grad = None
        mm(a, w.transpose(-2, -1)).backward(go)

    r["fwd_bwd_us"] = eager_us(lambda: step(lambda x, b_t: _to_mxfp8_then_scaled_grouped_mm(x, b_t, offs)), replays)
    r["bf16_fwd_bwd_us"] = eager_us(lambda: step(lambda x, b_t: torch._grouped_mm(x, b_t, offs=offs, out_dtype=torch.bfloat16)), replays)
    r["speedup_vs_bf16"] = r["bf16_fwd_bwd_us"] / r["fwd_bwd_us"]
    a.grad = w.grad = None
    with torch.no_grad():
        r["fwd_us"] = eager_us(lambda: _to_mxfp8_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs), replays)
        r["cast_go_rowwise_us"] = eager_us(lambda: ops.mxfp8_quantize(go), replays)
        r["cast_w_along_n_us"] = eager_us(lambda: ops.mxfp8_quantize_3d(w), replays)
        g_q, g_s = ops.mxfp8_quantize(go)
        w_q, w_s = ops.mxfp8_quantize_3d(w)
        w_q, w_s = w_q.transpose(-2, -1), w_s.contiguous()
        r["dgrad_us"] = eager_us(lambda: ops.mxfp8_grouped_mm(g_q, g_s, w_q, w_s, offs), replays)
        del g_q, g_s, w_q, w_s
        r["cast_go_colwise_us"] = eager_us(lambda: ops.mxfp8_quantize_colwise(go), replays)
        r["cast_a_colwise_us"] = eager_us(lambda: ops.mxfp8_quantize_colwise(a), replays)
        g_t, g_ts = ops.mxfp8_quantize_colwise(go)
        x_t, x_ts = ops.mxfp8_quantize_colwise(a)
        r["wgrad_us"] = eager_us(lambda: ops.mxfp8_grouped_mm_wgrad(g_t, g_ts, x_t, x_ts, offs, n, k), replays)
    r["wgrad_fp8_peak_fraction"] = 2.0 * m * n * k / (r["wgrad_us"] * 1e-6) / roofline.get_specs()["fp8_peak_tops"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=7, help="timed calls per figure (the median is recorded; at least 5)")
    ap.add_argument("--cells", default=",".join(CELLS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.replays < 5:
        ap.error("--replays must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_mxfp8_grouped_bwd.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None
    for name in args.cells.split(","):
        rec = json.dumps(cell(name, dev, args.replays))
        print(rec, flush=True)
        if out:
            out.write(rec + "\n")
            out.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
