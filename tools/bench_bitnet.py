#!/usr/bin/env python3
"""BitNet b1.58: the casts as HBM streams next to the eager chains, bs = 1 decode on the Llama-3-8B shapes next to the int8
dynamic linear, int4 and bf16 F.linear, both matmul forms forced over M (the seam is read from that sweep), and the training module forward +
backward at M = 8192 next to bf16 nn.Linear and the same module on _unpack_i2_in_i8 + torch._int_mm.

Operands rotate through copies worth 512 MiB (cold: twice the last-level cache); device events around windows of calls, the families of a cell
alternating; the median over --replays windows and (max - min) / median as the spread.  One JSON line per cell.
    python tools/bench_bitnet.py [--replays 5] [--out profiles/bitnet.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
from ao_amd import ops  # noqa: E402
from ao_amd.prototype import quantized_training as Q  # noqa: E402

COLD_BYTES = 512 << 20
WINDOW_US = 20e3
SWEEP_M = (1, 2, 4, 8, 16, 32, 64, 128, 256, 1024, 4096)
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


def eager_weight_cast(w):
    scale = w.float().abs().mean()
    return Q._pack_i2_in_i8((w.float() / scale.clip(1e-5)).round().clip(-1, 1).to(torch.int8)), scale


def eager_act_cast(x):
    scale = x.abs().amax(1) / 127
    inv = 1.0 / scale.float().clip(1e-5)
    return (x.float() * inv.view(-1, 1)).round().clip(-128, 127).to(torch.int8), scale


class EagerBitNetLinear(torch.autograd.Function):
    """The reference's module in eager ops: the chains above, an int8 copy of the weight, torch._int_mm."""

    @staticmethod
    def forward(ctx, x, w):
        a, rs = eager_act_cast(x)
        packed, scale = eager_weight_cast(w)
        ts = scale.to(w.dtype)
        ctx.save_for_backward(a, rs, packed, ts)
        return (torch._int_mm(a, Q._unpack_i2_in_i8(packed).T) * ts * rs.view(-1, 1)).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        a, rs, packed, ts = ctx.saved_tensors
        return (g @ Q._unpack_i2_in_i8(packed).to(g.dtype)) * ts, g.T @ (a * rs.view(-1, 1))


def emit(out, rec, r, base=None):
    for k, (us, spread) in r.items():
        rec[k + "_us"], rec[k + "_spread"] = round(us, 2), round(spread, 4)
    if base:
        rec.update({f"{k}_vs_{base}": round(r[base][0] / r[k][0], 3) for k in r if k != base})
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")


def casts(out, replays):
    n, k, m = 14336, 4096, 8192
    c = copies(2 * n * k)
    ws = [torch.randn(n, k, device=DEV, dtype=torch.bfloat16) * 0.02 for _ in range(c)]
    scale = ops.bitnet_absmean(ws[0])
    r = alternate({"absmean": lambda i: ops.bitnet_absmean(ws[i % c]), "absmean_eager": lambda i: ws[i % c].float().abs().mean(),
                   "weight_cast": lambda i: ops.bitnet_quantize_weight(ws[i % c], scale), "weight_cast_eager": lambda i: eager_weight_cast(ws[i % c])},
                  replays)
    emit(out, {"cell": "weight_casts", "N": n, "K": k, "absmean_tbps": round(2 * n * k / r["absmean"][0] * 1e-6, 3),
               "weight_cast_tbps": round(2.25 * n * k / r["weight_cast"][0] * 1e-6, 3)}, r)
    ps = [ops.bitnet_quantize_weight(w, scale) for w in ws]
    del ws
    r = alternate({"dequantize": lambda i: ops.bitnet_dequantize(ps[i % c]), "dequantize_eager": lambda i: Q._unpack_i2_in_i8(ps[i % c]).to(torch.bfloat16)},
                  replays)
    emit(out, {"cell": "dequantize", "N": n, "K": k, "dequantize_tbps": round(2.25 * n * k / r["dequantize"][0] * 1e-6, 3)}, r)
    del ps
    c = copies(2 * m * k)
    xs = [torch.randn(m, k, device=DEV, dtype=torch.bfloat16) for _ in range(c)]
    r = alternate({"act_cast": lambda i: ops.bitnet_quantize_act(xs[i % c]), "act_cast_eager": lambda i: eager_act_cast(xs[i % c])}, replays)
    emit(out, {"cell": "act_cast", "M": m, "K": k, "act_cast_tbps": round(3 * m * k / r["act_cast"][0] * 1e-6, 3)}, r)


def packed_weights(n, k, c):
    ts = torch.tensor(0.02, device=DEV, dtype=torch.bfloat16)
    return [torch.randint(-128, 128, (n, k // 4), device=DEV, dtype=torch.int8) & 0x55 for _ in range(c)], ts  # fields 0 / 1: valid codes


def decode(out, replays):
    for name, n, k in bench.LLAMA3_8B_UNMERGED:
        c = copies(n * k // 4)
        ps, ts = packed_weights(n, k, c)
        w = [torch.randn(n, k, device=DEV, dtype=torch.bfloat16) * 0.02 for _ in range(copies(2 * n * k))]
        w8 = [ops.int8_quantize_rowwise(w[0]) for _ in range(copies(n * k))]
        w4 = [ops.int4_quantize_tinygemm(w[0], 128) for _ in range(copies(n * k // 2))]
        x = torch.randn(1, k, device=DEV, dtype=torch.bfloat16)
        a, rs = ops.bitnet_quantize_act(x)
        r = alternate({"bitnet_linear": lambda i: ops.bitnet_linear(x, ps[i % c], ts), "bitnet_mm": lambda i: ops.bitnet_mm(a, ps[i % c], rs, ts),
                       "int8_dynamic": lambda i: ops.int8_linear(x, *w8[i % len(w8)]), "int4": lambda i: ops.weight_int4pack_mm(x, w4[i % len(w4)][0], 128, w4[i % len(w4)][1]),
                       "bf16": lambda i: F.linear(x, w[i % len(w)])}, replays)
        emit(out, {"cell": "decode_bs1", "shape": name, "N": n, "K": k, "bitnet_mm_weight_tbps": round(n * k / 4 / r["bitnet_mm"][0] * 1e-6, 3)}, r, "bf16")
        del ps, w, w8, w4


def forms(out, replays):
    for name, n, k in (("o", 4096, 4096), ("gate", 14336, 4096)):
        c = copies(n * k // 4)
        ps, ts = packed_weights(n, k, c)
        seam = None
        for m in SWEEP_M:
            a, rs = ops.bitnet_quantize_act(torch.randn(m, k, device=DEV, dtype=torch.bfloat16))
            r = alternate({"stream": lambda i: ops.bitnet_mm(a, ps[i % c], rs, ts, None, ops.BITNET_MM_STREAM),
                           "tiled": lambda i: ops.bitnet_mm(a, ps[i % c], rs, ts, None, ops.BITNET_MM_TILED)}, replays)
            if seam is None and r["tiled"][0] < r["stream"][0]:
                seam = m
            emit(out, {"cell": "forms", "shape": name, "M": m, "N": n, "K": k, "tiled_tops": round(2.0 * m * n * k / r["tiled"][0] * 1e-6, 1)}, r)
        emit(out, {"cell": "forms_seam", "shape": name, "first_M_where_tiled_is_ahead": seam}, {})


def training(out, replays):
    m = 8192
    for name, n, k in (("o", 4096, 4096), ("gate", 14336, 4096)):
        lin = torch.nn.Linear(k, n, bias=False, device=DEV, dtype=torch.bfloat16)
        bit = torch.nn.Linear(k, n, bias=False, device=DEV, dtype=torch.bfloat16)
        bit.weight = torch.nn.Parameter(Q.BitNetTrainingLinearWeight(bit.weight.detach()))
        w = lin.weight.detach().clone().requires_grad_()
        xs = [torch.randn(m, k, device=DEV, dtype=torch.bfloat16, requires_grad=True) for _ in range(4)]
        g = torch.randn(m, n, device=DEV, dtype=torch.bfloat16)

        def step(f):
            def run(i):
                f(xs[i % 4]).backward(g)
            return run

        r = alternate({"bitnet": step(bit), "bf16": step(lin), "eager_int_mm": step(lambda x: EagerBitNetLinear.apply(x, w))}, replays)
        emit(out, {"cell": "train_fwd_bwd", "shape": name, "M": m, "N": n, "K": k}, r, "bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitnet.jsonl"))
    args = ap.parse_args()
    with open(args.out, "w") as out:
        with torch.no_grad():
            casts(out, args.replays)
            decode(out, args.replays)
            forms(out, args.replays)
        training(out, args.replays)


if __name__ == "__main__":
    main()
