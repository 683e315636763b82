#!/usr/bin/env python3
"""AWQ's scale search: AWQObserver.calculate_qparams on the fused error kernel next to the same search written as the
reference writes it (prototype/awq/core.py:59-87) in eager ops of this library, on the Llama-3-8B linear shapes, g = 128, R = 20.

Every cell runs in a process of its own under a time limit (--cell-timeout); the parent never opens the GPU, and stops at the first cell
that does not exit cleanly.  Per cell (weights bf16 [N, K] ~ 0.02 N(0, 1), inputs with per-channel magnitudes exp(N(0, 1))):
  kernel_us        ops.awq_scaled_error at the chunk's R (core.AWQ_SEARCH_BYTES decides it), device events around a window of calls over
                   four copies of W in rotation (cold inputs), median window;  kernel_tbps = (2 + 4 R) N K bytes / that time
  fq_us, fq_tbps   ops.qat_int4_fake_quantize on the same tensors in the same process, 4 N K bytes: the yardstick stream
  search_ms        calculate_qparams() whole, host clock around a call that ends in a synchronise, median of --replays;
                   search_kernel_ms / search_matmul_ms: its launches and its matmuls alone, summed over the chunks (device events);
                   search_rest_ms: what is left (the table, x_mean, the multiply-and-sum, the argmin)
  eager_ms_<rows>  the reference's loop on stored inputs of 2048 and of 16384 rows: per ratio W * s, Int4Tensor.from_hp (with its compute
                   re-layout), two F.linear over all rows, .item();  same_pick_<rows>: whether it picks the ratio the fused search picks from
                   the Gram matrix of the same inputs;  speedup_<rows> = eager_ms / search_ms
  observe_us       one AWQObserver.forward of 2048 rows (device events, median window)
    python tools/bench_awq.py [--replays 3] [--shape NxK] [--no-eager] [--out profiles/awq.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336)]
GROUP = 128
RATIOS = 20
ROWS = (2048, 16384)


def window_us(fn, calls, replays):
    """Median over `replays` windows of `calls` calls fn(i), per call; one untimed window first."""
    import torch

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


def host_ms(fn, replays):
    """Median host time of fn(), which must leave the device idle (it ends in a synchronise here)."""
    import torch

    times = []
    for _ in range(replays):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        del out
    return statistics.median(times)


def eager_search(W, X, g, ratios):
    """core.py:59-87 as the reference writes it, on this library's Int4Tensor; returns the index of the ratio it picks"""
    import torch
    import torch.nn.functional as F

    from ao_amd.quantization.int4_plain_tensor import Int4Tensor

    x_max = X.abs().view(-1, X.shape[-1]).mean(0)
    best_loss, best = float("inf"), 0
    for i in range(ratios):
        ratio = i * 1 / ratios
        scales = x_max.pow(ratio).to(W.dtype).clamp(min=1e-4).view(-1)
        scales = scales / (scales.max() * scales.min()).sqrt()
        w = Int4Tensor.from_hp((W * scales).contiguous(), [1, g])
        orig_out = F.linear(X, W)
        q_out = F.linear(X / scales, w)
        loss = (orig_out - q_out).pow(2).mean().item()
        if loss < best_loss:
            best, best_loss = i, loss
    return best


def cell(n, k, replays, no_eager):
    import torch

    from ao_amd import ops
    from ao_amd.prototype.awq import AWQObserver, core
    from ao_amd.quantization.config import Int4WeightOnlyConfig

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    gen = torch.Generator(device=dev).manual_seed(0)
    W = (torch.randn(n, k, device=dev, generator=gen) * 0.02).to(torch.bfloat16)
    mag = torch.exp(torch.randn(k, device=dev, generator=gen))
    X = {rows: (torch.randn(rows, k, device=dev, generator=gen) * mag).to(torch.bfloat16) for rows in ROWS}
    base = Int4WeightOnlyConfig(group_size=GROUP, int4_packing_format="plain")
    rec = {"kind": "cell", "N": n, "K": k, "group": GROUP, "ratios": RATIOS, "replays": replays, "search_bytes": core.AWQ_SEARCH_BYTES}

    obs = {}
    for rows in ROWS:
        obs[rows] = AWQObserver(W, None, base, RATIOS)
        for r0 in range(0, rows, 2048):
            obs[rows](X[rows][r0:r0 + 2048], None)
    o = obs[ROWS[0]]
    o.calculate_qparams()  # warm-up: code objects, BLAS workspaces
    S = o.scales
    chunk = max(1, core.AWQ_SEARCH_BYTES // (8 * n * k))
    chunks = [min(chunk, RATIOS - r0) for r0 in range(0, RATIOS, chunk)]
    rec["chunks"] = chunks

    # the kernel alone, and the yardstick stream
    sets = [W.clone() for _ in range(4)]
    kernel_ms = matmul_ms = 0.0
    for rc in sorted(set(chunks), reverse=True):
        D = torch.empty((rc, n, k), dtype=torch.float32, device=dev)
        us = window_us(lambda i: ops.awq_scaled_error(sets[i % 4], S[:rc], GROUP, out=D), 8, replays)
        if rc == chunks[0]:
            rec["kernel_R"], rec["kernel_us"], rec["kernel_tbps"] = rc, us, (2 + 4 * rc) * n * k / (us * 1e-6) / 1e12
        mm = window_us(lambda i: torch.matmul(D.view(-1, k), o.gram), 4, replays)
        kernel_ms += us * 1e-3 * chunks.count(rc)
        matmul_ms += mm * 1e-3 * chunks.count(rc)
        if rc == chunks[0]:
            rec["matmul_us"], rec["matmul_tflops"] = mm, 2.0 * rc * n * k * k / (mm * 1e-6) / 1e12
        del D
        torch.cuda.empty_cache()
    rec["fq_us"] = window_us(lambda i: ops.qat_int4_fake_quantize(sets[i % 4], GROUP), 8, replays)
    rec["fq_tbps"] = 4 * n * k / (rec["fq_us"] * 1e-6) / 1e12

    rec["search_ms"] = host_ms(o.calculate_qparams, replays)
    rec["search_kernel_ms"], rec["search_matmul_ms"] = kernel_ms, matmul_ms
    rec["search_rest_ms"] = rec["search_ms"] - kernel_ms - matmul_ms
    rec["best_index"] = int(o.best_index)

    xs = [X[2048].clone() for _ in range(4)]
    rec["observe_us"] = window_us(lambda i: o(xs[i % 4], None), 8, replays)
    rec["observe_tflops"] = 2.0 * 2048 * k * k / (rec["observe_us"] * 1e-6) / 1e12

    if not no_eager:
        with torch.no_grad():
            eager_search(W[:256].contiguous(), X[2048][:256], GROUP, 2)  # warm-up
            for rows in ROWS:
                obs[rows].calculate_qparams()
                fused_pick = int(obs[rows].best_index)
                eager_pick = eager_search(W, X[rows], GROUP, RATIOS)
                rec[f"eager_ms_{rows}"] = host_ms(lambda: eager_search(W, X[rows], GROUP, RATIOS), max(1, replays - 1))
                rec[f"fused_pick_{rows}"], rec[f"eager_pick_{rows}"] = fused_pick, eager_pick
                rec[f"same_pick_{rows}"] = fused_pick == eager_pick
                rec[f"speedup_{rows}"] = rec[f"eager_ms_{rows}"] / rec["search_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=3)
    ap.add_argument("--shape", default=None, help="one shape NxK instead of the four")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cell-timeout", type=int, default=240, help="seconds a cell's process may take")
    ap.add_argument("--cell", default=None, help=argparse.SUPPRESS)  # the child's mode: measure one NxK and print its JSON line
    args = ap.parse_args()

    if args.cell:
        import torch

        if not torch.cuda.is_available():
            sys.exit("bench_awq.py measures on the GPU: no device visible")
        n, k = (int(v) for v in args.cell.split("x"))
        print(json.dumps(cell(n, k, args.replays, args.no_eager)), flush=True)
        return

    out = open(args.out, "a") if args.out else None
    shapes = [tuple(int(v) for v in args.shape.split("x"))] if args.shape else SHAPES
    for n, k in shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", f"{n}x{k}", "--replays", str(args.replays)] + (["--no-eager"] if args.no_eager else [])
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.cell_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"bench_awq.py: the cell {n}x{k} ran past its {args.cell_timeout} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"bench_awq.py: the cell {n}x{k} ended with status {done.returncode}; nothing more is started")
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
