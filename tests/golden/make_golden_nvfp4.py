"""Generate tests/golden/nvfp4.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_nvfp4.py

Everything runs on the CPU: nvfp4_quantize / NVFP4Tensor.to_nvfp4, dequantize, per_tensor_amax_to_scale, quantize_ with
NVFP4WeightOnlyConfig and the reference's own weight-only F.linear.  bf16 tensors are stored as uint16 bit patterns, codes and e4m3 scales
as uint8, per-tensor scales as fp32.

  cast_*     a seeded 12 x 64 matrix whose rows span 2^-14 .. 2^12
  edge_*     16-element blocks, one a row: zeros, -0.0, every rounding tie of e2m1 and its bf16 neighbours, amax below / at / above the
             points where the e4m3 scale rounds, amax that saturates the scale at 448, amax below the scale's floor, bf16 subnormals
  nonf_*     blocks holding Inf and NaN
             each cast three times: _none (no per-tensor scale), _given (p = 0.0123), _dyn (p = max|x| / 2688 of that matrix)
  deq_*      dequantize() bf16 bits of the cast_ tensors without and with the given p (not a power of two: both fp32 products round)
  w48_*      quantize_(Linear(128, 48), NVFP4WeightOnlyConfig()): the weight, qdata, the SWIZZLED scale it stores, the row-major scale of
             the same cast and the per-tensor scale
  lin_*      weight-only F.linear outputs (bias and no bias, with and without a power-of-two per-tensor scale) on exact-sum inputs:
             integer x, |x| <= 8, any e2m1 codes, block scales in {1/4, 1/2, 1, 2}
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GIVEN_P = 0.0123


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def bf(v):
    return torch.tensor(v, dtype=torch.float32).to(torch.bfloat16)


def nextafter_bf16(t, up):
    b = t.view(torch.int16).to(torch.int32)
    step = torch.where((t.float() >= 0) == up, 1, -1)
    return (b + step).to(torch.int16).view(torch.bfloat16)


def edge_blocks():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    t = bf([v for x in ties for v in (x, -x)] + [6.0, -6.0])  # amax 6: scale 1, r = 1
    rows = [torch.zeros(16, dtype=torch.bfloat16), -torch.zeros(16, dtype=torch.bfloat16), t]
    for up in (False, True):
        n = nextafter_bf16(t, up)
        n[14], n[15] = 6.0, -6.0
        rows.append(n)
    filler = bf([0.5, -1.0, 1.5, -2.0, 3.0, -0.25, 0.75, 0.0, -0.0, 1.25, -1.75, 2.5, -3.5, 4.0, 5.0])
    # block_scale = amax / 6 around the e4m3 ties 1.0625 (between 1 and 1.125: to even 1) and 1.1875 (to even 1.25), and 2^-6 (1 + 1/16)
    for amax in (6.34375, 6.375, 6.40625, 7.09375, 7.125, 7.15625, 0.099609375, 0.10009765625, 2688.0, 2720.0, 2816.0, 4000.0, 3.0e38,
                 0.09375, 0.01, 2.0 ** -20):
        rows.append(torch.cat([bf([amax]), (filler * (amax / 8)).to(torch.bfloat16)]))
    sub = torch.tensor([1, 2, 3, 0x7F, 0x40, 0x8001, 0x807F, 0x20, 0, 0x8000, 5, 0x8005, 0x11, 0x33, 0x55, 0x77], dtype=torch.int32)
    rows.append(sub.to(torch.int16).view(torch.bfloat16))                    # bf16 subnormals
    mixed = sub.to(torch.int16).view(torch.bfloat16).clone()
    mixed[3] = 2.0 ** -120
    rows.append(mixed)
    return torch.stack(rows)


def nonfinite_blocks():
    base = bf([0.5, -1.0, 1.5, -2.0, 3.0, -0.25, 0.75, 0.0, -0.0, 1.25, -1.75, 2.5, -3.5, 4.0, 5.0, -6.0])
    rows = []
    for idx, v in ((0, float("inf")), (5, float("-inf")), (2, float("nan")), (15, float("nan"))):
        r = base.clone()
        r[idx] = v
        rows.append(r)
    r = base.clone()
    r[1], r[9] = float("inf"), float("nan")
    rows.append(r)
    rows.append(base.clone())
    return torch.stack(rows)


def main():
    from torchao.prototype.mx_formats.inference_workflow import NVFP4WeightOnlyConfig
    from torchao.prototype.mx_formats.nvfp4_tensor import NVFP4Tensor, nvfp4_quantize, per_tensor_amax_to_scale
    from torchao.quantization import quantize_

    g = torch.Generator().manual_seed(0)
    out = {"given_p": np.float32(GIVEN_P)}
    mats = {
        "cast": (torch.randn(12, 64, generator=g) * torch.exp2(torch.arange(12, dtype=torch.float32) * 2.4 - 14).reshape(12, 1)).to(torch.bfloat16),
        "edge": edge_blocks(),
        "nonf": nonfinite_blocks(),
    }
    for name, x in mats.items():
        out[f"{name}_x"] = bits(x)
        dyn = per_tensor_amax_to_scale(torch.max(torch.abs(x)))
        out[f"{name}_dyn_p"] = dyn.numpy().copy()
        for mode, p in (("none", None), ("given", torch.tensor(GIVEN_P, dtype=torch.float32)), ("dyn", dyn)):
            s, q = nvfp4_quantize(x, 16, p)
            out[f"{name}_{mode}_q"] = q.view(torch.uint8).numpy().copy()
            out[f"{name}_{mode}_s"] = s.view(torch.uint8).numpy().copy()
            if name == "cast" and mode != "dyn":
                t = NVFP4Tensor.to_nvfp4(x, per_tensor_scale=p)
                assert torch.equal(t.qdata, q) and torch.equal(t.scale.view(torch.uint8), s.view(torch.uint8).reshape(t.scale.shape))
                out[f"deq_{mode}"] = bits(t.dequantize(torch.bfloat16))
    # quantize_ on a 48 x 128 weight: the swizzled scale the reference stores, and the row-major one of the same cast
    torch.manual_seed(1)
    lin = torch.nn.Linear(128, 48, bias=False).to(torch.bfloat16)
    w = lin.weight.detach().clone()
    quantize_(lin, NVFP4WeightOnlyConfig())
    t = lin.weight
    assert isinstance(t, NVFP4Tensor) and t.is_swizzled_scales and t.act_quant_kwargs is None
    s_rm, q = nvfp4_quantize(w, 16, t.per_tensor_scale)
    assert torch.equal(q, t.qdata)
    out["w48_w"], out["w48_q"] = bits(w), t.qdata.view(torch.uint8).numpy().copy()
    out["w48_scale_swizzled"] = t.scale.view(torch.uint8).numpy().copy()
    out["w48_scale_row_major"] = s_rm.view(torch.uint8).numpy().copy()
    out["w48_p"] = t.per_tensor_scale.numpy().copy()
    out["w48_deq"] = bits(t.dequantize(torch.bfloat16))
    # weight-only linear on exact-sum inputs
    M, N, K = 5, 24, 256
    x = torch.randint(-8, 9, (M, K), generator=g).to(torch.bfloat16)
    codes = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
    scale = torch.exp2(torch.randint(-2, 2, (N, K // 16), generator=g).to(torch.float32)).to(torch.float8_e4m3fn)
    bias = (torch.randn(N, generator=g) * 3).to(torch.bfloat16)
    out["lin_x"], out["lin_q"], out["lin_s"], out["lin_bias"] = bits(x), codes.numpy().copy(), scale.view(torch.uint8).numpy().copy(), bits(bias)
    out["lin_p"] = np.float32(2.0 ** -3)
    for tag, p in (("nop", None), ("p", torch.tensor(2.0 ** -3, dtype=torch.float32))):
        wt = NVFP4Tensor(codes, scale, 16, torch.bfloat16, p)
        assert wt.act_quant_kwargs is None
        out[f"lin_{tag}_y"] = bits(F.linear(x, wt, bias))
        out[f"lin_{tag}_y_nobias"] = bits(F.linear(x, wt))
    np.savez_compressed(os.path.join(HERE, "nvfp4.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
