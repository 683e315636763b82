"""Generate tests/golden/mx_linear.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the .npz:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_mx_linear.py

Everything runs on the CPU: to_mx(..., float4_e2m1fn_x2 / float8_e4m3fn, 32, mode, is_swizzled_scales=False), MXTensor.dequantize, and
quantize_ with MXDynamicActivationMXWeightConfig under KernelPreference.EMULATED.  bf16 tensors are stored as uint16 bit patterns,
codes and E8M0 scales as uint8.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def u8(t):
    return t.contiguous().view(torch.uint8).numpy().copy()


def bf(vals):
    return torch.tensor(vals, dtype=torch.float32).to(torch.bfloat16)


def edge_blocks():
    """[rows, 32] bf16 blocks at the edges of the fp4 cast."""
    rows = []
    ties = [6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, 0.0,
            -0.0, 0.1, 0.3, 0.6, 0.9, 1.1, 2.25, 2.75, 4.5, 5.5, 5.9, -4.5, -5.5, -5.9, 0.5, -0.5]
    rows.append(ties)
    rows.append([-0.0] * 32)
    rows.append([0.0] * 32)
    rng = np.random.default_rng(7)
    for k in (-133, -130, -127, -126, -100, -10, -1, 0, 1, 10, 100, 120, 125, 126, 127):
        for amax in (6.0 * 2.0 ** k,):
            a = float(torch.tensor(amax).to(torch.bfloat16).float())
            for t in (a, float(np.nextafter(np.float32(a), np.float32(np.inf))), float(np.nextafter(np.float32(a), np.float32(0)))):
                tb = float(torch.tensor(t, dtype=torch.float32).to(torch.bfloat16).float())
                # bf16 neighbours of amax
                ub = (torch.tensor([tb]).to(torch.bfloat16).view(torch.int16) + 1).view(torch.bfloat16).float().item()
                lb = (torch.tensor([tb]).to(torch.bfloat16).view(torch.int16) - 1).view(torch.bfloat16).float().item()
                for top in (tb, ub, lb):
                    if not np.isfinite(top) or top == 0:
                        continue
                    r = (rng.uniform(-1, 1, 32) * top).tolist()
                    r[int(rng.integers(32))] = -top if rng.integers(2) else top
                    rows.append(r)
    for tiny in (1e-40, 2.0 ** -133, 3e-39, 1e-38):
        rows.append((rng.uniform(-1, 1, 32) * tiny).tolist())
        rows[-1][0] = tiny
    rows.append([3.0e38] + (rng.uniform(-1, 1, 31) * 3e38).tolist())
    for special in (float("inf"), float("-inf"), float("nan")):
        r = rng.uniform(-4, 4, 32).tolist()
        r[5] = special
        rows.append(r)
    r = [float("nan")] * 32
    r[3] = -2.0
    rows.append(r)
    return bf(rows)


def main():
    from torchao.prototype.mx_formats.config import ScaleCalculationMode
    from torchao.prototype.mx_formats.inference_workflow import MXDynamicActivationMXWeightConfig
    from torchao.prototype.mx_formats.mx_tensor import MXTensor, to_mx
    from torchao.quantization import quantize_
    from torchao.quantization.quantize_.common.kernel_preference import KernelPreference

    out = {}
    g = torch.Generator().manual_seed(0)
    seeded = torch.cat([torch.randn(16, 256, generator=g) * s for s in (1.0, 1e-3, 37.0, 3e4)]).to(torch.bfloat16)
    edges = edge_blocks()
    out["seeded_x"] = bits(seeded)
    out["edge_x"] = bits(edges)
    for mode_name, mode in (("floor", ScaleCalculationMode.FLOOR), ("rceil", ScaleCalculationMode.RCEIL)):
        for name, x in (("seeded", seeded), ("edge", edges)):
            for elem, tag in ((torch.float4_e2m1fn_x2, "fp4"), (torch.float8_e4m3fn, "fp8")):
                s, d = to_mx(x, elem, 32, mode, is_swizzled_scales=False)
                out[f"{name}_{tag}_{mode_name}_q"] = u8(d)
                out[f"{name}_{tag}_{mode_name}_s"] = u8(s)
    # MXTensor.dequantize (bf16) of the seeded casts
    for elem, tag in ((torch.float4_e2m1fn_x2, "fp4"), (torch.float8_e4m3fn, "fp8")):
        t = MXTensor.to_mx(seeded, elem, 32, scaling_mode=ScaleCalculationMode.RCEIL)
        out[f"dequant_{tag}"] = bits(t.dequantize(torch.bfloat16))
        te = MXTensor.to_mx(edges, elem, 32, scaling_mode=ScaleCalculationMode.RCEIL)
        out[f"dequant_edge_{tag}"] = bits(te.dequantize(torch.bfloat16))
    # EMULATED linears through quantize_ (the reference's own path), with and without bias
    x = (torch.randn(8, 128, generator=g)).to(torch.bfloat16)
    w = (torch.randn(48, 128, generator=g) * 0.05).to(torch.bfloat16)
    b = (torch.randn(48, generator=g) * 0.1).to(torch.bfloat16)
    out["lin_x"], out["lin_w"], out["lin_b"] = bits(x), bits(w), bits(b)
    for elem, tag in ((torch.float4_e2m1fn_x2, "fp4"), (torch.float8_e4m3fn, "fp8")):
        for has_bias in (False, True):
            lin = torch.nn.Linear(128, 48, bias=has_bias, dtype=torch.bfloat16)
            with torch.no_grad():
                lin.weight.copy_(w)
                if has_bias:
                    lin.bias.copy_(b)
            cfg = MXDynamicActivationMXWeightConfig(activation_dtype=elem, weight_dtype=elem, kernel_preference=KernelPreference.EMULATED)
            quantize_(lin, cfg)
            with torch.no_grad():
                y = lin(x)
            out[f"lin_{tag}_{'bias' if has_bias else 'nobias'}"] = bits(y)
            if not has_bias:
                out[f"lin_{tag}_w_scale_shape"] = np.array(lin.weight.scale.shape, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "mx_linear.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
