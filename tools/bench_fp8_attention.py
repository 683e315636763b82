#!/usr/bin/env python3
"""FP8 attention: the per-head cast, the flash-attention kernel and fp8_sdpa end to end, next to bf16
F.scaled_dot_product_attention in the same process, windows alternating.

Shapes: Llama-3-8B prefill (Hq 32, Hkv 8, D 128, S 2048 and 8192, causal), a diffusion-style case (24 heads, D 128, S 4608, not causal) and
D 64 at S 1024 (the reference test's shape).  Inputs are four copies in rotation (cold: 4 x the working set), [B, S, H, D] memory seen as
[B, H, S, D]; device events around windows of calls; the median over --replays windows and (max - min) / median as the spread.
Per shape one JSON line:
  cast_us, kernel_us, fp8_sdpa_us, bf16_sdpa_us (+ *_spread)
  kernel_tflops   4 B Hq Sq Skv D / kernel_us (halved when causal);  peak_share: of the 5.0 PFLOP/s dense fp8 MFMA peak of the datasheet
  ratio_kernel, ratio_end_to_end   bf16_sdpa_us / kernel_us and / fp8_sdpa_us (below 1: the FP8 path is slower)
    python tools/bench_fp8_attention.py [--replays 5] [--out profiles/fp8_attention.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, B, Hq, Hkv, S, D, causal
SHAPES = [("llama3_8b_prefill_2k", 1, 32, 8, 2048, 128, True), ("llama3_8b_prefill_8k", 1, 32, 8, 8192, 128, True),
          ("diffusion_4608", 1, 24, 24, 4608, 128, False), ("d64_s1024", 2, 8, 8, 1024, 64, False)]
FP8_PEAK_TFLOPS = 5000.0
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
    calls = []
    for fn in fns.values():
        one_window(fn, 3)
        calls.append(max(5, min(500, int(WINDOW_US / max(one_window(fn, 5), 1e-3)))))
    times = {name: [] for name in fns}
    for _ in range(replays):
        for name, fn in fns.items():
            times[name].append(one_window(fn, min(calls)))
    return {name: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_attention.jsonl"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F

    from ao_amd import ops
    from ao_amd.prototype.attention import fp8_sdpa

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    with open(args.out, "w") as out:
        for name, B, Hq, Hkv, S, D, causal in SHAPES:
            def views(h):
                return [torch.randn(B, S, h, D, device=dev, generator=gen).to(torch.bfloat16).transpose(1, 2) for _ in range(4)]

            qs, ks, vs = views(Hq), views(Hkv), views(Hkv)
            codes = [ops.fp8_attn_quantize(qs[i], ks[i], vs[i]) for i in range(4)]
            r = alternate({
                "cast": lambda i: ops.fp8_attn_quantize(qs[i % 4], ks[i % 4], vs[i % 4]),
                "kernel": lambda i: ops.fp8_attn_fwd(*codes[i % 4], is_causal=causal),
                "fp8_sdpa": lambda i: fp8_sdpa(qs[i % 4], ks[i % 4], vs[i % 4], is_causal=causal),
                "bf16_sdpa": lambda i: F.scaled_dot_product_attention(qs[i % 4], ks[i % 4], vs[i % 4], is_causal=causal, enable_gqa=Hq != Hkv),
            }, args.replays)
            flops = 4.0 * B * Hq * S * S * D * (0.5 if causal else 1.0)
            tflops = flops / r["kernel"][0] * 1e-6
            rec = {"shape": name, "B": B, "Hq": Hq, "Hkv": Hkv, "S": S, "D": D, "causal": causal}
            for k, (us, spread) in r.items():
                rec[k + "_us"], rec[k + "_spread"] = round(us, 2), round(spread, 4)
            rec.update(kernel_tflops=round(tflops, 1), peak_share=round(tflops / FP8_PEAK_TFLOPS, 4),
                       ratio_kernel=round(r["bf16_sdpa"][0] / r["kernel"][0], 3), ratio_end_to_end=round(r["bf16_sdpa"][0] / r["fp8_sdpa"][0], 3))
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")


if __name__ == "__main__":
    main()
