"""Generate tests/golden/fp8_block.npz and tests/golden/fp8_block_configs.json by importing the REFERENCE (torchao) in the build
container.  Run once, commit both:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_fp8_block.py

Everything runs on the CPU: Float8Tensor.from_hp with PerBlock([128, 128]) (weights) and PerBlock([1, 128]) (activations), kernel_choice
"torch", dequantize() and an aten.slice of the weight.  The reference's blockwise GEMM is a Triton kernel and does not run here: no
output of it is recorded.  bf16 tensors are stored as uint16 bit patterns, e4m3 codes as uint8, scales as float32.
  w  [256, 384]: seeded; block (1, 0) all zero (scale 0, NaN codes); block (0, 2) holds 3e38 next to values near 1e-3 (they flush to 0)
  x  [7, 384] seeded, [6, 384] edge rows (a zero block, a saturating value beside tiny ones, +-0, subnormals, the bf16 maximum),
     [3, 5, 384] seeded 3-D
"""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def main():
    from torchao.core.config import config_to_dict
    from torchao.quantization import Float8DynamicActivationFloat8WeightConfig, PerBlock
    from torchao.quantization.quantize_.workflows.float8.float8_tensor import Float8Tensor

    g = torch.Generator().manual_seed(0)
    out = {}
    w = (torch.randn(256, 384, generator=g) * 0.05).to(torch.bfloat16)
    w[128:256, 0:128] = 0
    w[0:128, 256:384] = (torch.randn(128, 128, generator=g) * 1e-3).to(torch.bfloat16)
    w[5, 300] = 3e38
    wt = Float8Tensor.from_hp(w, granularity=PerBlock([128, 128]))
    assert list(wt.block_size) == [128, 128] and tuple(wt.scale.shape) == (2, 3)
    out["w"], out["w_q"], out["w_s"] = bits(w), wt.qdata.view(torch.uint8).numpy().copy(), wt.scale.to(torch.float32).numpy().copy()
    out["w_dequant"] = bits(wt.dequantize())
    sl = wt[128:256, 128:384]
    out["w_slice_q"], out["w_slice_s"] = sl.qdata.contiguous().view(torch.uint8).numpy().copy(), sl.scale.to(torch.float32).numpy().copy()
    out["w_slice_dequant"] = bits(sl.dequantize())

    x = (torch.randn(7, 384, generator=g) * torch.exp2(torch.randint(-3, 4, (7, 1), generator=g).float())).to(torch.bfloat16)
    edge = (torch.randn(6, 384, generator=g) * 0.5).to(torch.bfloat16)
    edge[0, 0:128] = 0
    edge[1, 128:256] = (torch.randn(128, generator=g) * 1e-4).to(torch.bfloat16)
    edge[1, 130] = -2e38
    edge[2, 0] = 0.0
    edge[2, 1] = -0.0
    edge[3, 256:384] = torch.tensor(1e-40).to(torch.bfloat16)
    edge[3, 257] = 1e-39
    edge[4, 5] = torch.finfo(torch.bfloat16).max
    edge[5, 0:128] = 448.0
    x3 = (torch.randn(3, 5, 384, generator=g) * 2.0).to(torch.bfloat16)
    for name, t in (("seeded", x), ("edge", edge), ("x3d", x3)):
        q = Float8Tensor.from_hp(t, granularity=PerBlock([1, 128]))
        assert tuple(q.scale.shape) == (*t.shape[:-1], 3)
        out[f"{name}_x"], out[f"{name}_q"] = bits(t), q.qdata.view(torch.uint8).numpy().copy()
        out[f"{name}_s"] = q.scale.to(torch.float32).numpy().copy()
    np.savez_compressed(os.path.join(HERE, "fp8_block.npz"), **out)
    configs = {"Float8DynamicActivationFloat8WeightConfig_block": config_to_dict(
        Float8DynamicActivationFloat8WeightConfig(granularity=[PerBlock([1, 128]), PerBlock([128, 128])]))}
    with open(os.path.join(HERE, "fp8_block_configs.json"), "w") as fh:
        json.dump(configs, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print({k: v.shape for k, v in out.items()})
    print(json.dumps(configs))


if __name__ == "__main__":
    main()
