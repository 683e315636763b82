#!/usr/bin/env python3
"""Forward + backward of the float8 rowwise MoE grouped GEMM next to bf16 autograd of torch._grouped_mm and the MXFP8
grouped GEMM, in one process, on the cells of tools/bench_mxfp8_grouped_bwd.py:

    cell               E    W [N, K]         tokens per expert
    mixtral_w1         8    [14336, 4096]    2048
    deepseek_v3_ep8    32   [2048, 7168]     2048   (one EP-8 rank's routed experts)

Per cell (eager calls between two device events, the median of the replays).  A figure of one launch sequence is taken on input
buffers rotated through copies that together exceed twice the 256 MiB last-level cache, so every call streams its input from HBM:
  1. the jagged cast (memset + amax + scales + codes) of grad_out and of A: jagged_cast_go_us / jagged_cast_a_us; the plain column cast
     of the same tensor, ops.fp8_train_amax(cols) + ops.fp8_train_cast(col) (the same bytes moved, one scale vector instead of E):
     colwise_cast_*_us; the per-group loop of torch ops (amax, scale, multiply, clamp, cast, transposed copy): eager_group_loop_*_us;
  2. wgrad_us: ops.fp8_grouped_mm_wgrad; wgrad_dense_loop_us: E calls of ops.fp8_scaled_mm on per-group operands cast beforehand (each
     group's codes contiguous, so the slices are legal); mx_wgrad_us: ops.mxfp8_grouped_mm_wgrad on the same shape;
     wgrad_fp8_peak_fraction = 2 M N K / wgrad_us over the dense fp8 MFMA peak (ao_amd/roofline.py);
  3. fwd_bwd_us: _to_fp8_rowwise_then_scaled_grouped_mm (no padding: the groups are multiples of 16) on tensors that require grad, then
     out.backward(grad_out); bf16_fwd_bwd_us: torch._grouped_mm through autograd; mx_fwd_bwd_us: _to_mxfp8_then_scaled_grouped_mm;
     every launch of the step alone (cast_*_us, fwd_gemm_us, dgrad_us, wgrad_us) and cast_share = the casts' sum over the launches' sum.
    python tools/bench_fp8_grouped_training.py [--replays 7] [--cells mixtral_w1,deepseek_v3_ep8] [--out profiles/fp8_grouped_training.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ao_amd import ops, roofline  # noqa: E402
from ao_amd.prototype.fp8_grouped_training import _to_fp8_rowwise_then_scaled_grouped_mm  # noqa: E402
from ao_amd.prototype.mx import _to_mxfp8_then_scaled_grouped_mm  # noqa: E402

CELLS = {"mixtral_w1": (8, 14336, 4096, 2048), "deepseek_v3_ep8": (32, 2048, 7168, 2048)}
ROTATE_BYTES = 2 * 256 << 20  # the copies of an input together: twice the last-level cache


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


class Rotating:
    """Copies of a tensor, handed out in turn."""

    def __init__(self, t):
        n = max(2, -(-ROTATE_BYTES // (t.numel() * t.element_size())))
        self.copies = [t] + [t.clone() for _ in range(n - 1)]
        self.i = 0

    def next(self):
        self.i = (self.i + 1) % len(self.copies)
        return self.copies[self.i]


def eager_group_cast(x, ends):
    """torch_to_float8_per_group_colwise in torch ops, the codes stored transposed."""
    q_t = torch.empty((x.shape[1], x.shape[0]), dtype=torch.float8_e4m3fn, device=x.device)
    scales = []
    lo = 0
    for hi in ends:
        sub = x[lo:hi].float()
        s = (448.0 / sub.abs().amax(dim=0, keepdim=True).double().clamp(min=1e-12)).float()
        s = torch.exp2(torch.floor(torch.log2(s)))
        q_t[:, lo:hi] = (sub * s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).t()
        scales.append(s)
        lo = hi
    return q_t, torch.cat(scales)


def cell(name, dev, replays):
    e, n, k, per = CELLS[name]
    m = e * per
    a = torch.randn(m, k, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    w = (torch.randn(e, n, k, device=dev, dtype=torch.bfloat16) * 0.02).requires_grad_(True)
    go = torch.randn(m, n, device=dev, dtype=torch.bfloat16) * 0.01
    ends = [per * (i + 1) for i in range(e)]
    offs = torch.tensor(ends, dtype=torch.int32, device=dev)
    r = {"cell": name, "E": e, "N": n, "K": k, "M_total": m, "replays": replays}

    def step(mm):
        a.grad = w.grad = None
        mm(a, w.transpose(-2, -1)).backward(go)

    # 3. the step, three ways, in the same process
    r["fwd_bwd_us"] = eager_us(lambda: step(lambda x, b_t: _to_fp8_rowwise_then_scaled_grouped_mm(x, b_t, offs, pad_token_groups_for_grouped_mm=False)), replays)
    r["bf16_fwd_bwd_us"] = eager_us(lambda: step(lambda x, b_t: torch._grouped_mm(x, b_t, offs=offs, out_dtype=torch.bfloat16)), replays)
    r["mx_fwd_bwd_us"] = eager_us(lambda: step(lambda x, b_t: _to_mxfp8_then_scaled_grouped_mm(x, b_t, offs)), replays)
    r["speedup_vs_bf16"] = r["bf16_fwd_bwd_us"] / r["fwd_bwd_us"]
    r["speedup_vs_mxfp8"] = r["mx_fwd_bwd_us"] / r["fwd_bwd_us"]
    a.grad = w.grad = None
    with torch.no_grad():
        ad, wd = a.detach(), w.detach()
        ra, rgo = Rotating(ad), Rotating(go)
        # 1. the jagged cast against the plain column cast and the eager loop
        for tag, rot in (("go", rgo), ("a", ra)):
            r[f"jagged_cast_{tag}_us"] = eager_us(lambda: ops.fp8_train_quantize_group_colwise_t(rot.next(), offs, True), replays)
            r[f"colwise_cast_{tag}_us"] = eager_us(lambda: ops.fp8_train_quantize_colwise_t(rot.next(), True), replays)
            r[f"eager_group_loop_{tag}_us"] = eager_us(lambda: eager_group_cast(rot.next(), ends), replays)
        # the other launches of the step
        w2 = wd.view(e * n, k)
        r["cast_a_rowwise_us"] = eager_us(lambda: ops.fp8_train_quantize_rowwise(ra.next(), True), replays)
        r["cast_w_rowwise_us"] = eager_us(lambda: ops.fp8_train_quantize_rowwise(w2, True), replays)
        r["cast_go_rowwise_us"] = eager_us(lambda: ops.fp8_train_quantize_rowwise(rgo.next(), True), replays)
        r["cast_w_3d_t_us"] = eager_us(lambda: ops.fp8_train_quantize_colwise_t_3d(wd, True), replays)
        del ra, rgo
        a_q, _, a_inv = ops.fp8_train_quantize_rowwise(ad, True)
        w_q, _, w_inv = ops.fp8_train_quantize_rowwise(w2, True)
        r["fwd_gemm_us"] = eager_us(lambda: ops.fp8_grouped_mm(a_q, a_inv, w_q.view(e, n, k), w_inv.view(e, n), offs), replays)
        del a_q, w_q
        g_q, _, g_inv = ops.fp8_train_quantize_rowwise(go, True)
        w_t, _, w_tinv = ops.fp8_train_quantize_colwise_t_3d(wd, True)
        r["dgrad_us"] = eager_us(lambda: ops.fp8_grouped_mm(g_q, g_inv, w_t, w_tinv, offs), replays)
        del g_q, w_t
        # 2. the weight gradient
        g_t, _, g_tinv = ops.fp8_train_quantize_group_colwise_t(go, offs, True)
        x_t, _, x_tinv = ops.fp8_train_quantize_group_colwise_t(ad, offs, True)
        r["wgrad_us"] = eager_us(lambda: ops.fp8_grouped_mm_wgrad(g_t, g_tinv, x_t, x_tinv, offs, n, k), replays)
        del g_t, x_t
        groups = []
        for i in range(e):
            gq, _, gi = ops.fp8_train_quantize_colwise_t(go[i * per:(i + 1) * per], True)   # [N, per]
            xq, _, xi = ops.fp8_train_quantize_colwise_t(ad[i * per:(i + 1) * per], True)   # [K, per]
            groups.append((gq, xq.t(), gi, xi))
        r["wgrad_dense_loop_us"] = eager_us(lambda: [ops.fp8_scaled_mm(gq, xq_t, gi, xi) for gq, xq_t, gi, xi in groups], replays)
        del groups
        mg_t, mg_s = ops.mxfp8_quantize_colwise(go)
        mx_t, mx_s = ops.mxfp8_quantize_colwise(ad)
        r["mx_wgrad_us"] = eager_us(lambda: ops.mxfp8_grouped_mm_wgrad(mg_t, mg_s, mx_t, mx_s, offs, n, k), replays)
    r["wgrad_fp8_peak_fraction"] = 2.0 * m * n * k / (r["wgrad_us"] * 1e-6) / roofline.get_specs()["fp8_peak_tops"]
    casts = sum(r[key] for key in ("cast_a_rowwise_us", "cast_w_rowwise_us", "cast_go_rowwise_us", "cast_w_3d_t_us", "jagged_cast_go_us",
                                    "jagged_cast_a_us"))
    launches = casts + r["fwd_gemm_us"] + r["dgrad_us"] + r["wgrad_us"]
    r["launches_sum_us"] = launches
    r["cast_share"] = casts / launches
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
        sys.exit("bench_fp8_grouped_training.py measures on the GPU: no device visible")
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
