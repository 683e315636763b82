#!/usr/bin/env python3
"""GPTQ's convert step in one process: gptq_quantize on the fused block kernel next to the same arithmetic written as a chain
of eager torch ops column by column -- the reference's structure (prototype/gptq/api.py:446-532: per column about a dozen launches on
[N, 1] slices) on this library's primitives -- on the Llama-3-8B linear shapes.

  cells   formats int4 (group 128), int8 (per row), nvfp4; weights bf16 [N, K] of (4096, 4096), (6144, 4096), (14336, 4096), (4096, 14336);
          H from 2048 random correlated tokens; block size 256.  Per cell:
            fused_ms        gptq_quantize(H, W, config): dead columns, damping, the three Cholesky calls, per block one launch and one
                            matmul, the result tensor.  Host clock around a call that ends in a synchronise; median of --replays.
            factor_ms       the dead columns, damping and Cholesky calls alone (both paths run them)
            eager_ms        the same steps with the column loop as eager torch ops (eager_quantize below); median of --eager-replays
            speedup_vs_eager = eager_ms / fused_ms;  loop_speedup = (eager_ms - factor_ms) / (fused_ms - factor_ms)
            codes_equal     the share of the fused result's code bytes the eager chain reproduces (both start from the same Hinv)
            block_us        ops.gptq_block alone on one 256-column block (device events around a window of calls, median window)
  hessian GPTQObserverTensor.update_2d of 2048 tokens at K = 4096 and 14336 (one addmm_): device events, median window
    python tools/bench_gptq.py [--replays 5] [--eager-replays 2] [--shape NxK] [--format int4] [--no-eager] [--out profiles/gptq.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ao_amd import ops  # noqa: E402
from ao_amd.prototype import NVFP4DynamicActivationNVFP4WeightConfig  # noqa: E402
from ao_amd.prototype.gptq import GPTQConfig, GPTQObserverTensor, gptq_quantize  # noqa: E402
from ao_amd.quantization.config import Int4WeightOnlyConfig, Int8WeightOnlyConfig  # noqa: E402

SHAPES = [(4096, 4096), (6144, 4096), (14336, 4096), (4096, 14336)]
TOKENS = 2048
BLOCK = 256
INT4_G = 128
BASES = {"int4": lambda: Int4WeightOnlyConfig(group_size=INT4_G), "int8": Int8WeightOnlyConfig, "nvfp4": NVFP4DynamicActivationNVFP4WeightConfig}
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


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


def host_ms(fn, replays):
    """Median host time of fn(), which must leave the device idle (it ends in a synchronise here)."""
    times = []
    for _ in range(replays):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        del out
    return statistics.median(times), times


def inputs(n, k, dev, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    W = (torch.randn(n, k, device=dev, generator=gen) * 0.02).to(torch.bfloat16)
    x = torch.randn(TOKENS, k, device=dev, generator=gen)
    x = x + 0.5 * x.roll(1, dims=1) * torch.logspace(-0.5, 0.5, k, device=dev)  # correlated columns of unequal variance
    x[:, 11] = 0  # a dead column
    obs = GPTQObserverTensor.from_hp(W)
    obs.update_2d(x.to(torch.bfloat16))
    return W, obs.hessian.clone()


def factorize(H, W, percdamp):
    """prototype/gptq/api.py:392-403, as ao_amd/prototype/gptq/api.py runs it"""
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    W[:, dead] = 0
    damp = percdamp * torch.mean(torch.diag(H))
    diag = torch.arange(H.shape[0], device=H.device)
    H[diag, diag] += damp
    H = torch.linalg.cholesky(H)
    H = torch.cholesky_inverse(H)
    return torch.linalg.cholesky(H, upper=True).contiguous()


# ---- the column loop as eager torch ops: the reference's structure, one small launch per operation per column --------------------------
def _e2m1_codes(v):
    a = v.abs()
    c = torch.zeros_like(v, dtype=torch.uint8)
    for hit in (a > 0.25, a >= 0.75, a > 1.25, a >= 1.75, a > 2.5, a >= 3.5, a > 5.0):  # ties to the even code
        c += hit.to(torch.uint8)
    return c | (torch.signbit(v).to(torch.uint8) << 3)


def eager_quantize(H, W, fmt, percdamp=0.01):
    """gptq_quantize with the column loop in eager torch ops; returns the packed codes (int8: the codes)."""
    n, k = W.shape
    lut = torch.tensor(E2M1, device=W.device)
    if fmt == "int8":
        row_scale = ops.int8_quantize_rowwise(W)[1]  # Int8Tensor.from_hp's scale [N, 1]: this library's cast
        inv = 1.0 / row_scale
    elif fmt == "nvfp4":
        p = ops.nvfp4_amax_scale(W)
    # torch divides a device tensor by a Python scalar as a multiplication by the reciprocal: a tensor divisor keeps the division
    fifteen = torch.tensor(15.0, device=W.device)
    Hinv = factorize(H, W, percdamp)
    g = {"int4": INT4_G, "int8": BLOCK, "nvfp4": 16}[fmt]
    codes = torch.empty((n, k), dtype=torch.int8 if fmt != "nvfp4" else torch.uint8, device=W.device)
    for k0 in range(0, k, BLOCK):
        end = min(k0 + BLOCK, k)
        blk = W[:, k0:end]
        h = Hinv[k0:end, k0:end]
        err = torch.zeros(n, end - k0, dtype=torch.float32, device=W.device)
        for g0 in range(0, end - k0, g):
            cols = blk[:, g0:g0 + g].float()
            if fmt == "int4":
                mx, mn = cols.amax(dim=1, keepdim=True), cols.amin(dim=1, keepdim=True)
                scale = torch.clamp(mx - mn, min=1e-6) / fifteen
                zero = mn + scale * 8
                m = zero - scale * 8
            elif fmt == "nvfp4":
                _, s8 = ops.nvfp4_quantize(blk[:, g0:g0 + g].contiguous(), p)  # this library's cast: the block scales under p
                r = ((1.0 / p) / s8.to(torch.float32))
            for c in range(g0, min(g0 + g, end - k0)):
                w = blk[:, c].unsqueeze(1)
                if fmt == "int4":
                    q = w.float().sub(m).div(scale).round().clamp_(0, 15)
                    dq = q * scale + m
                elif fmt == "nvfp4":
                    dq = lut[_e2m1_codes(torch.clamp(w * r, -6.0, 6.0)).long()] / r
                else:
                    dq = torch.clamp(torch.round(w * inv), -128, 127) * row_scale
                e = (w - dq) / h[c, c]
                blk[:, c:] -= e.matmul(h[c, c:].unsqueeze(0))
                err[:, c] = e.flatten()
            # the final codes of the group's columns (api.py:537-569 does all of W at the end: the same values)
            cols = blk[:, g0:g0 + g].float()
            if fmt == "int4":
                codes[:, k0 + g0:k0 + g0 + g] = (cols.sub(m).div(scale).round().clamp_(0, 15) - 8).to(torch.int8)
            elif fmt == "nvfp4":
                codes[:, k0 + g0:k0 + g0 + g] = _e2m1_codes(torch.clamp(cols * r, -6.0, 6.0))
            else:
                codes[:, k0 + g0:k0 + g0 + g] = torch.clamp(torch.round(cols * inv), -128, 127).to(torch.int8)
        W[:, end:] -= err.matmul(Hinv[k0:end, end:])
    if fmt == "int8":
        return codes
    c = codes.to(torch.uint8) & 0xF
    return c[:, 0::2] | (c[:, 1::2] << 4)


def cell(n, k, fmt, dev, replays, eager_replays, no_eager):
    W0, H0 = inputs(n, k, dev)
    cfg = GPTQConfig("convert", BASES[fmt](), gptq_quantize_block_size=BLOCK)
    rec = {"kind": "cell", "format": fmt, "N": n, "K": k, "block": BLOCK, "group": {"int4": INT4_G, "int8": 0, "nvfp4": 16}[fmt], "tokens": TOKENS,
           "replays": replays, "launches_fused": 2 * (-(-k // BLOCK)) - 1}
    fused = gptq_quantize(H0.clone(), W0.clone(), cfg)  # warm-up: code objects, solver workspaces
    rec["fused_ms"], rec["fused_ms_all"] = host_ms(lambda: gptq_quantize(H0.clone(), W0.clone(), cfg), replays)
    rec["factor_ms"], _ = host_ms(lambda: factorize(H0.clone(), W0.clone(), cfg.percdamp), replays)
    # the block kernel alone: one 256-column block, fresh copies of W in rotation
    Hinv = factorize(H0.clone(), W0.clone(), cfg.percdamp)
    sets = [W0.clone() for _ in range(4)]
    qd = fused.qdata.clone()
    kw = {"int4": lambda: dict(group_size=INT4_G, scale=fused.scale.clone(), zero_point=fused.zero_point.clone()),
          "int8": lambda: dict(row_scale=fused.scale.reshape(-1).clone()),
          "nvfp4": lambda: dict(scale=fused.scale.clone(), per_tensor_scale=fused.per_tensor_scale.clone())}[fmt]()
    code = {"int4": ops.GPTQ_INT4, "int8": ops.GPTQ_INT8, "nvfp4": ops.GPTQ_NVFP4}[fmt]
    err = torch.empty((n, BLOCK), dtype=torch.float32, device=dev)
    rec["block_us"] = window_us(lambda i: ops.gptq_block(sets[i % 4], Hinv, 0, BLOCK, code, qd, err=err, **kw), 16, replays)
    if not no_eager:
        with torch.no_grad():
            eager_quantize(H0.clone()[:BLOCK, :BLOCK].contiguous(), W0.clone()[:256, :BLOCK].contiguous(), fmt)  # warm-up at one block
            got = eager_quantize(H0.clone(), W0.clone(), fmt)
            rec["codes_equal"] = float((got == fused.qdata.view(got.dtype)).float().mean().item())
            rec["eager_ms"], rec["eager_ms_all"] = host_ms(lambda: eager_quantize(H0.clone(), W0.clone(), fmt), eager_replays)
        rec["eager_replays"] = eager_replays
        rec["speedup_vs_eager"] = rec["eager_ms"] / rec["fused_ms"]
        rec["loop_speedup"] = (rec["eager_ms"] - rec["factor_ms"]) / max(rec["fused_ms"] - rec["factor_ms"], 1e-9)
    return rec


def hessian(k, dev, replays):
    obs = GPTQObserverTensor.from_hp(torch.zeros(16, k, device=dev, dtype=torch.bfloat16))
    xs = [torch.randn(TOKENS, k, device=dev).to(torch.bfloat16) for _ in range(4)]
    us = window_us(lambda i: obs.update_2d(xs[i % 4]), 16, replays)
    return {"kind": "hessian", "K": k, "tokens": TOKENS, "update_us": us, "tflops": 2.0 * TOKENS * k * k / (us * 1e-6) / 1e12, "replays": replays}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--eager-replays", type=int, default=2, help="timed runs of the eager chain (each takes seconds)")
    ap.add_argument("--shape", default=None, help="one shape NxK instead of the four")
    ap.add_argument("--format", default=None, choices=list(BASES))
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gptq.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    shapes = [tuple(int(v) for v in args.shape.split("x"))] if args.shape else SHAPES
    for n, k in shapes:
        for fmt in ([args.format] if args.format else list(BASES)):
            emit(cell(n, k, fmt, dev, args.replays, args.eager_replays, args.no_eager))
            torch.cuda.empty_cache()
    for k in sorted({k for _, k in shapes}):
        emit(hessian(k, dev, args.replays))


if __name__ == "__main__":
    main()
