#!/usr/bin/env python3
"""Forward + backward of the blockwise float8 MoE grouped GEMM next to bf16 autograd of torch._grouped_mm, the float8
rowwise grouped op and the MXFP8 grouped op, in one process, with the method of tools/bench_fp8_grouped_training.py:

    cell                  E    W [N, K]         tokens per expert
    deepseek_v3_ep8_w13   32   [2048, 7168]     2048   (one EP-8 rank's routed experts, gate / up)
    deepseek_v3_ep8_w2    32   [7168, 2048]     2048   (the same rank, down)
    mixtral_w1            8    [14336, 4096]    2048

Per cell (eager calls between two device events, the median of the replays).  A figure of one launch is taken on input buffers rotated
through copies that together exceed twice the 256 MiB last-level cache, so every call streams its input from HBM:
  1. cast_w_3d_us: ops.fp8_block_train_cast_weight_3d(w, transposed=None), both layouts from one read, and its HBM stream
     cast_w_3d_tbps = (2 + 1 + 1) bytes an element over the time; cast_w_2d_loop_us: E calls of ops.fp8_block_train_cast_weight(w[e],
     transposed=None), the same bytes;
  2. wgrad_us: ops.fp8_block_grouped_mm_wgrad on the column casts of all tokens; wgrad_dense_loop_us: E calls of ops.fp8_block_mm_wgrad
     on per-group operands made contiguous beforehand (the same tile loop, E launches); rowwise_wgrad_us: ops.fp8_grouped_mm_wgrad
     (float8 rowwise, one scale a column and group); wgrad_fp8_peak_fraction = 2 M N K / wgrad_us over the dense fp8 MFMA peak;
  3. fwd_bwd_us: _to_fp8_blockwise_then_scaled_grouped_mm (no padding: the groups are multiples of 128) on tensors that require grad,
     then out.backward(grad_out); padded_fwd_bwd_us: the same with the groups padded; bf16_fwd_bwd_us: torch._grouped_mm through
     autograd; rowwise_fwd_bwd_us: _to_fp8_rowwise_then_scaled_grouped_mm; mx_fwd_bwd_us: _to_mxfp8_then_scaled_grouped_mm; every launch
     of the step alone (cast_*_us, fwd_gemm_us, dgrad_us, wgrad_us) and cast_share = the casts' sum over the launches' sum.
    python tools/bench_fp8_block_grouped_training.py [--replays 7] [--cells ...] [--out profiles/fp8_block_grouped_training.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ao_amd import ops, roofline  # noqa: E402
from ao_amd.prototype.blockwise_fp8_grouped_training import _to_fp8_blockwise_then_scaled_grouped_mm  # noqa: E402
from ao_amd.prototype.fp8_grouped_training import _to_fp8_rowwise_then_scaled_grouped_mm  # noqa: E402
from ao_amd.prototype.mx import _to_mxfp8_then_scaled_grouped_mm  # noqa: E402

CELLS = {"deepseek_v3_ep8_w13": (32, 2048, 7168, 2048), "deepseek_v3_ep8_w2": (32, 7168, 2048, 2048), "mixtral_w1": (8, 14336, 4096, 2048)}
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


def cell(name, dev, replays):
    e, n, k, per = CELLS[name]
    m = e * per
    a = torch.randn(m, k, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    w = (torch.randn(e, n, k, device=dev, dtype=torch.bfloat16) * 0.02).requires_grad_(True)
    go = torch.randn(m, n, device=dev, dtype=torch.bfloat16) * 0.01
    offs = torch.tensor([per * (i + 1) for i in range(e)], dtype=torch.int32, device=dev)
    r = {"cell": name, "E": e, "N": n, "K": k, "M_total": m, "replays": replays}

    def step(mm):
        a.grad = w.grad = None
        mm(a, w.transpose(-2, -1)).backward(go)

    # 3. the step, five ways, in the same process
    block = lambda pad: lambda x, b_t: _to_fp8_blockwise_then_scaled_grouped_mm(x, b_t, offs, pad_token_groups_for_grouped_mm=pad)  # noqa: E731
    r["fwd_bwd_us"] = eager_us(lambda: step(block(False)), replays)
    r["padded_fwd_bwd_us"] = eager_us(lambda: step(block(True)), replays)
    r["bf16_fwd_bwd_us"] = eager_us(lambda: step(lambda x, b_t: torch._grouped_mm(x, b_t, offs=offs, out_dtype=torch.bfloat16)), replays)
    r["rowwise_fwd_bwd_us"] = eager_us(
        lambda: step(lambda x, b_t: _to_fp8_rowwise_then_scaled_grouped_mm(x, b_t, offs, pad_token_groups_for_grouped_mm=False)), replays)
    r["mx_fwd_bwd_us"] = eager_us(lambda: step(lambda x, b_t: _to_mxfp8_then_scaled_grouped_mm(x, b_t, offs)), replays)
    for other in ("bf16", "rowwise", "mx"):
        r[f"speedup_vs_{other}"] = r[f"{other}_fwd_bwd_us"] / r["fwd_bwd_us"]
    a.grad = w.grad = None
    with torch.no_grad():
        ad, wd = a.detach(), w.detach()
        # 1. the 3-D weight cast against the loop of 2-D casts
        rw = Rotating(wd)
        r["cast_w_3d_us"] = eager_us(lambda: ops.fp8_block_train_cast_weight_3d(rw.next(), transposed=None), replays)
        r["cast_w_3d_tbps"] = 4.0 * e * n * k / (r["cast_w_3d_us"] * 1e-6) / 1e12
        r["cast_w_2d_loop_us"] = eager_us(lambda: [ops.fp8_block_train_cast_weight(x, transposed=None) for x in rw.next()], replays)
        r["cast_w_plain_us"] = eager_us(lambda: ops.fp8_block_train_cast_weight_3d(rw.next(), transposed=False), replays)
        r["cast_w_t_us"] = eager_us(lambda: ops.fp8_block_train_cast_weight_3d(rw.next(), transposed=True), replays)
        del rw
        # the other casts of the step
        ra, rgo = Rotating(ad), Rotating(go)
        r["cast_a_rows_us"] = eager_us(lambda: ops.fp8_block_train_cast(ra.next(), rows=True, cols=False), replays)
        r["cast_a_cols_us"] = eager_us(lambda: ops.fp8_block_train_cast(ra.next(), rows=False, cols=True), replays)
        r["cast_go_both_us"] = eager_us(lambda: ops.fp8_block_train_cast(rgo.next(), rows=True, cols=True), replays)
        del ra, rgo
        (a_q, a_inv), (x_t, x_inv) = ops.fp8_block_train_cast(ad, rows=True, cols=True)
        (g_q, g_inv), (g_t, g_tinv) = ops.fp8_block_train_cast(go, rows=True, cols=True)
        (w_q, w_inv), (w_t, w_tinv) = ops.fp8_block_train_cast_weight_3d(wd, transposed=None)
        r["fwd_gemm_us"] = eager_us(lambda: ops.fp8_block_grouped_mm(a_q, a_inv, w_q, w_inv, offs), replays)
        r["dgrad_us"] = eager_us(lambda: ops.fp8_block_grouped_mm(g_q, g_inv, w_t, w_tinv, offs), replays)
        del a_q, g_q, w_q, w_t
        # 2. the weight gradient
        r["wgrad_us"] = eager_us(lambda: ops.fp8_block_grouped_mm_wgrad(g_t, g_tinv, x_t, x_inv, offs), replays)
        pb = per // 128
        groups = [(g_t[:, i * per:(i + 1) * per].contiguous(), g_tinv[i * pb:(i + 1) * pb], x_t[:, i * per:(i + 1) * per].contiguous(),
                   x_inv[i * pb:(i + 1) * pb]) for i in range(e)]
        same = all(torch.equal(ops.fp8_block_mm_wgrad(*groups[i]), ops.fp8_block_grouped_mm_wgrad(g_t, g_tinv, x_t, x_inv, offs)[i])
                   for i in (0, e - 1))
        r["wgrad_equals_dense_loop"] = bool(same)
        r["wgrad_dense_loop_us"] = eager_us(lambda: [ops.fp8_block_mm_wgrad(*g) for g in groups], replays)
        del groups, g_t, x_t
        j_t, _, j_inv = ops.fp8_train_quantize_group_colwise_t(go, offs, True)
        jx_t, _, jx_inv = ops.fp8_train_quantize_group_colwise_t(ad, offs, True)
        r["rowwise_wgrad_us"] = eager_us(lambda: ops.fp8_grouped_mm_wgrad(j_t, j_inv, jx_t, jx_inv, offs, n, k), replays)
    r["wgrad_vs_dense_loop"] = r["wgrad_dense_loop_us"] / r["wgrad_us"]
    r["wgrad_vs_rowwise"] = r["rowwise_wgrad_us"] / r["wgrad_us"]
    r["wgrad_fp8_peak_fraction"] = 2.0 * m * n * k / (r["wgrad_us"] * 1e-6) / roofline.get_specs()["fp8_peak_tops"]
    casts = sum(r[key] for key in ("cast_a_rows_us", "cast_a_cols_us", "cast_go_both_us", "cast_w_plain_us", "cast_w_t_us"))
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
        sys.exit("bench_fp8_block_grouped_training.py measures on the GPU: no device visible")
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
