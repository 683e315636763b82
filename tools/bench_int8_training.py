#!/usr/bin/env python3
"""Int8 mixed-precision training on the Llama-3-8B shapes at M = 8192: the cast (rows, columns, both) as an HBM stream next to
the same chain in eager torch ops; int8_train_mm in each of the three flag pairs of a linear as a share of the int8 MFMA peak, next to
ops.int8_scaled_mm (the contraction-innermost kernel of the inference path) on the same codes; the module forward + backward next to bf16
nn.Linear autograd and Float8Linear (rowwise).

Operands rotate through copies worth 512 MiB (cold: twice the last-level cache); device events around windows of calls, the families of a cell
alternating; the median over --replays windows and (max - min) / median as the spread.  One JSON line per cell.
    python tools/bench_int8_training.py [--replays 5] [--out profiles/int8_training.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from ao_amd import ops  # noqa: E402
from ao_amd.float8 import Float8LinearConfig, convert_to_float8_training  # noqa: E402
from ao_amd.prototype import quantized_training as Q  # noqa: E402
from ao_amd.quantization import quantize_  # noqa: E402

COLD_BYTES = 512 << 20
WINDOW_US = 20e3
M = 8192
DEV = torch.device("cuda", 0)


def one_window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def alternate(fns, replays):
    calls = []
    for fn in fns.values():
        one_window(fn, 3)
        calls.append(max(5, min(400, int(WINDOW_US / max(one_window(fn, 5), 1e-3)))))
    times = {name: [] for name in fns}
    for _ in range(replays):
        for name, fn in fns.items():
            times[name].append(one_window(fn, min(calls)))
    return {name: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for name, t in times.items()}


def copies(nbytes):
    return max(2, min(64, -(-COLD_BYTES // nbytes)))


def eager_cast(t):
    scale = t.abs().amax(1) / 127
    inv = 1.0 / scale.float().clip(1e-12)
    return (t.float() * inv.view(-1, 1)).round().clip(-128, 127).to(torch.int8), scale


def emit(out, rec, r, base=None):
    for k, (us, spread) in r.items():
        rec[k + "_us"], rec[k + "_spread"] = round(us, 2), round(spread, 4)
    if base:
        rec.update({f"{k}_vs_{base}": round(r[base][0] / r[k][0], 3) for k in r if k != base})
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")


def casts(out, replays):
    for c_cols in (4096, 14336):
        c = copies(2 * M * c_cols)
        xs = [torch.randn(M, c_cols, device=DEV, dtype=torch.bfloat16) for _ in range(c)]
        r = alternate({"rows": lambda i: ops.int8_train_quantize(xs[i % c]), "cols": lambda i: ops.int8_train_quantize(xs[i % c], rows=False, cols=True),
                       "both": lambda i: ops.int8_train_quantize(xs[i % c], cols=True), "rows_eager": lambda i: eager_cast(xs[i % c]),
                       "cols_eager": lambda i: eager_cast(xs[i % c].T)[0].contiguous()}, replays)
        n = M * c_cols  # bytes moved: rows 2 + 1 a element, columns 2 + 2 + 1, both 2 + 2 + 1 + 1
        emit(out, {"cell": "cast", "R": M, "C": c_cols, "rows_tbps": round(3 * n / r["rows"][0] * 1e-6, 3), "cols_tbps": round(5 * n / r["cols"][0] * 1e-6, 3),
                   "both_tbps": round(6 * n / r["both"][0] * 1e-6, 3), "rows_vs_eager": round(r["rows_eager"][0] / r["rows"][0], 2),
                   "cols_vs_eager": round(r["cols_eager"][0] / r["cols"][0], 2)}, r)
        del xs


def gemms(out, replays):
    for name, n_w, k_w in bench.LLAMA3_8B_UNMERGED:
        # (GEMM, rows of A, rows of B, contraction, flags)
        for gemm, m, n, kc, a_t, b_t in (("out", M, n_w, k_w, False, False), ("grad_input", M, k_w, n_w, False, True), ("grad_weight_t", k_w, n_w, M, True, True)):
            c = copies(m * kc + n * kc)
            a = [torch.randint(-128, 128, (kc, m) if a_t else (m, kc), device=DEV, dtype=torch.int8) for _ in range(c)]
            b = [torch.randint(-128, 128, (kc, n) if b_t else (n, kc), device=DEV, dtype=torch.int8) for _ in range(c)]
            sa, sb = torch.rand(m, device=DEV).to(torch.bfloat16), torch.rand(n, device=DEV).to(torch.bfloat16)
            # the inference kernel takes the contraction innermost only: its operands are the same codes, transposed outside the timing
            a_nt = [t.T.contiguous() if a_t else t for t in a]
            b_nt = [t.T.contiguous() if b_t else t for t in b]
            sa32, sb32 = sa.float(), sb.float()
            r = alternate({"int8_train_mm": lambda i: ops.int8_train_mm(a[i % c], b[i % c], sa, sb, a_t=a_t, b_t=b_t),
                           "int8_scaled_mm_nt": lambda i: ops.int8_scaled_mm(a_nt[i % c], sa32, b_nt[i % c], sb32)}, replays)
            tops = 2.0 * m * n * kc / r["int8_train_mm"][0] * 1e-6
            emit(out, {"cell": "mm", "shape": name, "gemm": gemm, "M": m, "N": n, "Kc": kc, "a_t": a_t, "b_t": b_t, "kernel": ops.int8_train_mm_kernel_name(a_t, b_t),
                       "tops": round(tops, 1), "frac_of_int8_peak": round(tops / bench.MFMA_8BIT_PEAK_TOPS, 3),
                       "nt_frac_of_int8_peak": round(2.0 * m * n * kc / r["int8_scaled_mm_nt"][0] * 1e-6 / bench.MFMA_8BIT_PEAK_TOPS, 3)}, r, "int8_scaled_mm_nt")
            del a, b, a_nt, b_nt


def training(out, replays):
    for name, n, k in bench.LLAMA3_8B_UNMERGED:
        def linear():
            return torch.nn.Linear(k, n, bias=False, device=DEV, dtype=torch.bfloat16)

        lin, i8, f8 = linear(), linear(), torch.nn.Sequential(linear())
        quantize_(i8, Q.Int8MixedPrecisionTrainingConfig())
        convert_to_float8_training(f8, config=Float8LinearConfig.from_recipe_name("rowwise"))
        xs = [torch.randn(M, k, device=DEV, dtype=torch.bfloat16, requires_grad=True) for _ in range(4)]
        g = torch.randn(M, n, device=DEV, dtype=torch.bfloat16)

        def step(f):
            def run(i):
                f(xs[i % 4]).backward(g)
            return run

        r = alternate({"int8_mixed": step(i8), "bf16": step(lin), "float8_rowwise": step(f8)}, replays)
        emit(out, {"cell": "train_fwd_bwd", "shape": name, "M": M, "N": n, "K": k}, r, "bf16")
        del lin, i8, f8, xs, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8_training.jsonl"))
    args = ap.parse_args()
    with open(args.out, "w") as out:
        with torch.no_grad():
            casts(out, args.replays)
            gemms(out, args.replays)
        training(out, args.replays)


if __name__ == "__main__":
    main()
