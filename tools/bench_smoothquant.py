#!/usr/bin/env python3
"""SmoothQuant's run-time route and calibration kernels.

F.linear on an Int8Tensor with a per-input-feature act_pre_scale (what SmoothQuantConfig's convert produces), the NEW route -- the
pre-scale folded into the activation cast (ops.int8_quantize_*_prescaled) -- next to the PARENT route -- `x * act_pre_scale` as a torch
multiply, then the unscaled linear -- in the same process, windows alternating, on N x K in {4096 x 4096, 14336 x 4096, 4096 x 14336} and
M in {1, 2, 16, 256, 4096}, for the dynamic PerRow and the static PerTensor activation.  Every shape runs in a process of its own under a
time limit (--cell-timeout); the parent never opens the GPU, and stops at the first cell that does not exit cleanly.

Per (base, M), device events around windows of calls over four copies of the activation in rotation; a window is sized to about 30 ms:
  new_us, parent_us      median over --replays windows, per call
  new_spread, parent_spread   (max - min) / median over those windows: the run-to-run spread a difference has to exceed
  speedup                parent_us / new_us;   ahead: new_us < parent_us by more than the larger spread
  same_bytes             the two routes' outputs are the same bytes (asserted)
  saved_bytes            4 M K: the bf16 write and read of the product the new route does not make
  at M = 1 (dynamic PerRow) also cast_mm_us: the pre-scaled cast + ao_int8_scaled_mm, the form the route does NOT take at one row
Once per process: kernel A (ops.sq_col_absmax_update) on bf16 [2048, 4096] next to x.abs().amax(0) into the same state, and kernel B
(ops.sq_smoothed_amax_update) next to (x / s).abs().amax(); us and TB/s of the 2 M K input bytes.
    python tools/bench_smoothquant.py [--replays 5] [--shape NxK] [--out profiles/smoothquant.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336)]
MS = (1, 2, 16, 256, 4096)
WINDOW_US = 30e3


def one_window(fn, calls):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def alternate(fns, replays):
    """{name: (median us, spread)} of the named fn(i), their windows alternating; one untimed window each first, which also sizes the window"""
    calls = {}
    for name, fn in fns.items():
        one_window(fn, 5)
        calls[name] = max(10, min(1000, int(WINDOW_US / max(one_window(fn, 10), 1e-3))))
    n = min(calls.values())  # the same number of calls for every route
    times = {name: [] for name in fns}
    for _ in range(replays):
        for name, fn in fns.items():
            times[name].append(one_window(fn, n))
    return {name: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for name, t in times.items()}, n


def calibration_kernels(replays):
    import torch

    from ao_amd import ops

    dev = torch.device("cuda", 0)
    m, k = 2048, 4096
    gen = torch.Generator(device=dev).manual_seed(1)
    xs = [(torch.randn(m, k, device=dev, generator=gen) * torch.exp(torch.randn(k, device=dev, generator=gen))).to(torch.bfloat16) for _ in range(4)]
    s = torch.exp2(torch.rand(k, device=dev, generator=gen) * 12 - 6).to(torch.bfloat16)
    state, state_t = torch.zeros(k, dtype=torch.float32, device=dev), torch.zeros(k, dtype=torch.float32, device=dev)
    amax, amax_t = torch.zeros(1, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)

    def torch_a(i):
        torch.maximum(state_t, xs[i % 4].abs().amax(0).float(), out=state_t)

    def torch_b(i):
        torch.maximum(amax_t, (xs[i % 4] / s).abs().amax().float().reshape(1), out=amax_t)

    ra, na = alternate({"kernel": lambda i: ops.sq_col_absmax_update(xs[i % 4], state), "torch": torch_a}, replays)
    rb, nb = alternate({"kernel": lambda i: ops.sq_smoothed_amax_update(xs[i % 4], s, amax), "torch": torch_b}, replays)
    assert torch.equal(state, state_t) and torch.equal(amax, amax_t), "the kernels and the torch ops disagree"
    rec = {"kind": "calibration", "M": m, "K": k, "replays": replays}
    for tag, r, n in (("absmax", ra, na), ("smoothed_amax", rb, nb)):
        rec[f"{tag}_calls"] = n
        for name in ("kernel", "torch"):
            rec[f"{tag}_{name}_us"], rec[f"{tag}_{name}_spread"] = r[name]
        rec[f"{tag}_kernel_tbps"] = 2.0 * m * k / (r["kernel"][0] * 1e-6) / 1e12
        rec[f"{tag}_speedup"] = r["torch"][0] / r["kernel"][0]
    return rec


def cell(n, k, replays):
    import torch
    import torch.nn.functional as F

    from ao_amd import ops
    from ao_amd.quantization.granularity import PerRow, PerTensor
    from ao_amd.quantization.int8_tensor import Int8Tensor, QuantizeTensorToInt8Kwargs

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    gen = torch.Generator(device=dev).manual_seed(0)
    W = (torch.randn(n, k, device=dev, generator=gen) * 0.02).to(torch.bfloat16)
    mag = torch.exp(torch.randn(k, device=dev, generator=gen))
    pre = (1.0 / mag.sqrt()).to(torch.bfloat16)
    recs = []
    for base in ("dynamic_per_row", "static_per_tensor"):
        if base == "dynamic_per_row":
            w = Int8Tensor.from_hp(W, PerRow(), act_quant_kwargs=QuantizeTensorToInt8Kwargs(granularity=PerRow()))
        else:
            w = Int8Tensor.from_hp(W, PerRow(), act_quant_kwargs=QuantizeTensorToInt8Kwargs(granularity=PerTensor()),
                                   act_quant_scale=torch.full((1, 1), 0.05, dtype=torch.float32, device=dev))
        parent_w = Int8Tensor(w.qdata, w.scale, w.block_size, w.dtype_, w.act_quant_kwargs, None, None, None, w.act_quant_scale, None)
        w.act_pre_scale = pre
        for m in MS:
            xs = [(torch.randn(m, k, device=dev, generator=gen) * mag).to(torch.bfloat16) for _ in range(4)]
            fns = {"new": lambda i: F.linear(xs[i % 4], w), "parent": lambda i: F.linear(xs[i % 4] * pre, parent_w)}
            if m == 1 and base == "dynamic_per_row":
                fns["cast_mm"] = lambda i: ops.int8_scaled_mm(*ops.int8_quantize_rowwise_prescaled(xs[i % 4], pre), w.qdata, w._row_scale())
            with torch.no_grad():
                same = all(torch.equal(fn(0).view(torch.int16), fns["parent"](0).view(torch.int16)) for fn in fns.values())
                assert same, f"{base} M={m}: the routes' outputs differ"
                r, calls = alternate(fns, replays)
            rec = {"kind": "linear", "base": base, "N": n, "K": k, "M": m, "calls": calls, "replays": replays, "same_bytes": same,
                   "saved_bytes": 4 * m * k}
            for name in fns:
                rec[f"{name}_us"], rec[f"{name}_spread"] = r[name]
            rec["speedup"] = r["parent"][0] / r["new"][0]
            rec["ahead"] = bool(r["parent"][0] - r["new"][0] > max(r["new"][1], r["parent"][1]) * r["parent"][0])
            recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--shape", default=None, help="one shape NxK instead of the three")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cell-timeout", type=int, default=240, help="seconds a cell's process may take")
    ap.add_argument("--cell", default=None, help=argparse.SUPPRESS)  # the child's mode: NxK, or "calibration"; prints JSON lines
    args = ap.parse_args()

    if args.cell:
        import torch

        if not torch.cuda.is_available():
            sys.exit("bench_smoothquant.py measures on the GPU: no device visible")
        if args.cell == "calibration":
            print(json.dumps(calibration_kernels(args.replays)), flush=True)
        else:
            n, k = (int(v) for v in args.cell.split("x"))
            for rec in cell(n, k, args.replays):
                print(json.dumps(rec), flush=True)
        return

    out = open(args.out, "a") if args.out else None
    shapes = [tuple(int(v) for v in args.shape.split("x"))] if args.shape else SHAPES
    for name in ["calibration"] + [f"{n}x{k}" for n, k in shapes]:
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", name, "--replays", str(args.replays)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.cell_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"bench_smoothquant.py: the cell {name} ran past its {args.cell_timeout} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"bench_smoothquant.py: the cell {name} ended with status {done.returncode}; nothing more is started")
        for line in done.stdout.strip().splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()


if __name__ == "__main__":
    main()
