#!/usr/bin/env python3
"""Forward + backward of the NVFP4 MoE grouped GEMM next to bf16 autograd of torch._grouped_mm and the float8 rowwise,
blockwise float8 and MXFP8 grouped ops, in one process, with the method of tools/bench_fp8_block_grouped_training.py:

    cell                  E    W [N, K]         tokens per expert
    deepseek_v3_ep8_w13   32   [2048, 7168]     2048   (one EP-8 rank's routed experts, gate / up)
    deepseek_v3_ep8_w2    32   [7168, 2048]     2048   (the same rank, down)
    mixtral_w1            8    [14336, 4096]    2048

Per cell (eager calls between two device events, the median of the replays).  A figure of one launch is taken on input buffers rotated
through copies that together exceed twice the 256 MiB last-level cache, so every call streams its input from HBM:
  1. group_amax_us / group_cast_us (RTNE) / group_cast_sr_us: the two grouped casts of the activation as HBM streams (cast: 2 bytes read,
     2 x 0.5625 written an element), next to amax_loop_us / cast_loop_us: E dense calls on the groups' row slices;
     cast_w_3d_us next to cast_w_2d_loop_us, and weight_amax_3d_us;
  2. wgrad_us: ops.nvfp4_grouped_mm_wgrad on the column casts of all tokens; wgrad_dense_loop_us: E launches of ops.nvfp4_scaled_mm on
     per-group operands made contiguous beforehand (three sets of them in turn); wgrad_bf16_peak_fraction = 2 M N K / wgrad_us over
     the dense bf16 MFMA peak (the kernel multiplies decoded bf16);
  3. fwd_bwd_us: _to_nvfp4_rht_rs_then_scaled_grouped_mm on tensors that require grad, then out.backward(grad_out); bf16_fwd_bwd_us,
     rowwise_fwd_bwd_us, block_fwd_bwd_us, mx_fwd_bwd_us: the other recipes; fwd_gemm_us, dgrad_us: the scaled grouped mm alone, the
     codes of both operands rotated as in 1 and 2.
    python tools/bench_nvfp4_grouped_training.py [--replays 7] [--cells ...] [--out profiles/nvfp4_grouped_training.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ao_amd import ops, roofline  # noqa: E402
from ao_amd.prototype.blockwise_fp8_grouped_training import _to_fp8_blockwise_then_scaled_grouped_mm  # noqa: E402
from ao_amd.prototype.fp8_grouped_training import _to_fp8_rowwise_then_scaled_grouped_mm  # noqa: E402
from ao_amd.prototype.mx import _to_mxfp8_then_scaled_grouped_mm  # noqa: E402
from ao_amd.prototype.nvfp4_grouped_training import _to_nvfp4_rht_rs_then_scaled_grouped_mm  # noqa: E402
from ao_amd.prototype.nvfp4_training import DEFAULT_SIGN_VECTOR as SIGN, _amax_to_scale  # noqa: E402
from bench_fp8_block_grouped_training import CELLS, Rotating, eager_us  # noqa: E402


def cell(name, dev, replays):
    e, n, k, per = CELLS[name]
    m = e * per
    a = torch.randn(m, k, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    w = (torch.randn(e, n, k, device=dev, dtype=torch.bfloat16) * 0.02).requires_grad_(True)
    go = torch.randn(m, n, device=dev, dtype=torch.bfloat16) * 0.01
    offs = torch.tensor([per * (i + 1) for i in range(e)], dtype=torch.int32, device=dev)
    seed = torch.tensor([1234], dtype=torch.int64, device=dev)
    off = torch.tensor([7], dtype=torch.int64, device=dev)
    r = {"cell": name, "E": e, "N": n, "K": k, "M_total": m, "replays": replays}

    def step(mm):
        a.grad = w.grad = None
        mm(a, w.transpose(-2, -1)).backward(go)

    # 3. the step, five ways, in the same process
    r["fwd_bwd_us"] = eager_us(lambda: step(lambda x, b_t: _to_nvfp4_rht_rs_then_scaled_grouped_mm(x, b_t.transpose(-2, -1), SIGN, seed, offs)), replays)
    r["bf16_fwd_bwd_us"] = eager_us(lambda: step(lambda x, b_t: torch._grouped_mm(x, b_t, offs=offs, out_dtype=torch.bfloat16)), replays)
    r["rowwise_fwd_bwd_us"] = eager_us(
        lambda: step(lambda x, b_t: _to_fp8_rowwise_then_scaled_grouped_mm(x, b_t, offs, pad_token_groups_for_grouped_mm=False)), replays)
    r["block_fwd_bwd_us"] = eager_us(
        lambda: step(lambda x, b_t: _to_fp8_blockwise_then_scaled_grouped_mm(x, b_t, offs, pad_token_groups_for_grouped_mm=False)), replays)
    r["mx_fwd_bwd_us"] = eager_us(lambda: step(lambda x, b_t: _to_mxfp8_then_scaled_grouped_mm(x, b_t, offs)), replays)
    for other in ("bf16", "rowwise", "block", "mx"):
        r[f"speedup_vs_{other}"] = r[f"{other}_fwd_bwd_us"] / r["fwd_bwd_us"]
    a.grad = w.grad = None
    with torch.no_grad():
        ad, wd = a.detach(), w.detach()
        # 1. the casts as HBM streams, next to the loops of dense calls
        ra = Rotating(ad)
        amax = ops.nvfp4_train_group_amax(ad, offs, SIGN)
        r["group_amax_us"] = eager_us(lambda: ops.nvfp4_train_group_amax(ra.next(), offs, SIGN), replays)
        r["group_amax_tbps"] = 2.0 * m * k / (r["group_amax_us"] * 1e-6) / 1e12
        r["amax_loop_us"] = eager_us(lambda: [ops.nvfp4_train_amax(x, SIGN) for x in ra.next().split(per)], replays)
        r["group_cast_us"] = eager_us(lambda: ops.nvfp4_train_quantize_row_col_grouped(ra.next(), amax, offs, SIGN), replays)
        r["group_cast_tbps"] = (2.0 + 2 * 0.5625) * m * k / (r["group_cast_us"] * 1e-6) / 1e12
        r["group_cast_sr_us"] = eager_us(lambda: ops.nvfp4_train_quantize_row_col_grouped(ra.next(), amax, offs, SIGN, seed, off, off), replays)
        r["cast_loop_us"] = eager_us(lambda: [ops.nvfp4_train_quantize_row_col(x, amax[i], SIGN) for i, x in enumerate(ra.next().split(per))], replays)
        del ra
        rw = Rotating(wd)
        w_amax = ops.nvfp4_train_weight_amax_3d(wd)
        r["weight_amax_3d_us"] = eager_us(lambda: ops.nvfp4_train_weight_amax_3d(rw.next()), replays)
        r["cast_w_3d_us"] = eager_us(lambda: ops.nvfp4_train_quantize_weight_3d(rw.next(), w_amax), replays)
        r["cast_w_3d_tbps"] = (2.0 + 2 * 0.5625) * e * n * k / (r["cast_w_3d_us"] * 1e-6) / 1e12
        r["cast_w_2d_loop_us"] = eager_us(lambda: [ops.nvfp4_train_quantize_weight_2d(x, w_amax[i]) for i, x in enumerate(rw.next())], replays)
        del rw
        # the GEMMs of the step alone
        g_amax = ops.nvfp4_train_group_amax(go, offs, SIGN)
        x_cq, x_cs, x_rq, x_rs = ops.nvfp4_train_quantize_row_col_grouped(ad, amax, offs, SIGN)
        g_cq, g_cs, g_rq, g_rs = ops.nvfp4_train_quantize_row_col_grouped(go, g_amax, offs, SIGN, seed, off, off)
        w_q, w_s, wt_q, wt_s = ops.nvfp4_train_quantize_weight_3d(wd, w_amax)
        px, pxc, pg, pgc, pw = (_amax_to_scale(t).contiguous() for t in (amax[:, 1], amax[:, 0], g_amax[:, 1], g_amax[:, 0], w_amax))
        # (the codes of both operands of a GEMM rotate too; the scale bytes, an eighth of them, and the [E] scales stay)
        rx, rg, rwq, rwt = Rotating(x_rq), Rotating(g_rq), Rotating(w_q), Rotating(wt_q)
        r["fwd_gemm_us"] = eager_us(lambda: ops.nvfp4_scaled_grouped_mm(rx.next(), x_rs, rwq.next(), w_s, offs, px, pw), replays)
        r["dgrad_us"] = eager_us(lambda: ops.nvfp4_scaled_grouped_mm(rg.next(), g_rs, rwt.next(), wt_s, offs, pg, pw), replays)
        del x_rq, g_rq, w_q, wt_q, rx, rg, rwq, rwt
        # 2. the weight gradient
        rgc, rxc = Rotating(g_cq), Rotating(x_cq)
        r["wgrad_us"] = eager_us(lambda: ops.nvfp4_grouped_mm_wgrad(rgc.next(), g_cs, rxc.next(), x_cs, pgc, pxc, offs), replays)
        del rgc, rxc
        cut = lambda t, i, d: t[:, i * per // d:(i + 1) * per // d].contiguous()  # noqa: E731
        groups = [(cut(g_cq, i, 2), cut(g_cs, i, 16), cut(x_cq, i, 2), cut(x_cs, i, 16), pgc[i], pxc[i]) for i in range(e)]
        full = ops.nvfp4_grouped_mm_wgrad(g_cq, g_cs, x_cq, x_cs, pgc, pxc, offs)
        # (the two kernels add in different orders: the share of equal elements is recorded, not asserted)
        r["wgrad_equal_to_dense_loop"] = float((ops.nvfp4_scaled_mm(*groups[0]) == full[0]).float().mean())
        sets = [groups, [tuple(t.clone() for t in g) for g in groups], [tuple(t.clone() for t in g) for g in groups]]
        turn = [0]

        def dense_loop():
            turn[0] = (turn[0] + 1) % len(sets)
            return [ops.nvfp4_scaled_mm(*g) for g in sets[turn[0]]]

        r["wgrad_dense_loop_us"] = eager_us(dense_loop, replays)
    r["wgrad_vs_dense_loop"] = r["wgrad_dense_loop_us"] / r["wgrad_us"]
    r["wgrad_bf16_peak_fraction"] = 2.0 * m * n * k / (r["wgrad_us"] * 1e-6) / roofline.get_specs()["bf16_peak_tops"]
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
        sys.exit("bench_nvfp4_grouped_training.py measures on the GPU: no device visible")
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
