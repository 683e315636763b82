"""Generate tests/golden/wo8.npz and tests/golden/wo8_configs.json by importing the REFERENCE (torchao) in the build container.  Run once,
commit both:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_wo8.py

Everything runs on the CPU: Int8Tensor.from_hp / Float8Tensor with act_quant_kwargs=None and the reference's own F.linear, for PerRow and
PerTensor, with a bias.  Inputs whose sums are exact in fp32 in any order: integer-valued x with |x| <= 8 and K = 256; int8 codes as
from_hp gives them (|q| <= 127); e4m3 tensors built directly from integer codes |q| <= 15 with power-of-two scales that differ per row.
One float8 case has general from_hp scales and a one-hot x: its output is dequantize()[:, :16].T.  bf16 tensors are stored as uint16 bit
patterns, e4m3 codes as uint8.
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
M, N, K = 5, 24, 256


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def main():
    from torchao.core.config import config_to_dict
    from torchao.quantization import Float8WeightOnlyConfig, Int8WeightOnlyConfig, PerRow, PerTensor
    from torchao.quantization.quantize_.workflows.float8.float8_tensor import Float8Tensor
    from torchao.quantization.quantize_.workflows.int8.int8_tensor import Int8Tensor

    g = torch.Generator().manual_seed(0)
    out = {}
    x = torch.randint(-8, 9, (M, K), generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
    out["x"], out["w"], out["bias"] = bits(x), bits(w), bits(bias)
    for tag, gran in (("row", PerRow()), ("tensor", PerTensor())):
        t = Int8Tensor.from_hp(w, granularity=gran)
        assert t.act_quant_kwargs is None
        out[f"int8_{tag}_q"] = t.qdata.numpy().copy()
        out[f"int8_{tag}_s"] = t.scale.to(torch.float32).numpy().copy()
        out[f"int8_{tag}_y"] = bits(F.linear(x, t, bias))
        out[f"int8_{tag}_y_nobias"] = bits(F.linear(x, t))
        # e4m3 from integer codes and power-of-two scales
        codes = torch.randint(-15, 16, (N, K), generator=g).to(torch.float32).to(torch.float8_e4m3fn)
        if tag == "row":
            scale = torch.exp2(torch.arange(N, dtype=torch.float32) % 11 - 7).reshape(N, 1)
            block = [1, K]
        else:
            scale = torch.tensor([[2.0 ** -5]], dtype=torch.float32)
            block = [N, K]
        f = Float8Tensor(codes, scale, block_size=block, dtype=torch.bfloat16)
        assert f.act_quant_kwargs is None
        out[f"e4m3_{tag}_q"] = codes.view(torch.uint8).numpy().copy()
        out[f"e4m3_{tag}_s"] = scale.numpy().copy()
        out[f"e4m3_{tag}_y"] = bits(F.linear(x, f, bias))
        out[f"e4m3_{tag}_y_nobias"] = bits(F.linear(x, f))
    # general scales, one-hot activation
    f = Float8Tensor.from_hp(w, granularity=PerRow())
    eye = torch.eye(16, K, dtype=torch.bfloat16)
    y = F.linear(eye, f)
    assert torch.equal(y, f.dequantize()[:, :16].t())
    out["onehot_q"] = f.qdata.view(torch.uint8).numpy().copy()
    out["onehot_s"] = f.scale.to(torch.float32).numpy().copy()
    out["onehot_y"] = bits(y)
    out["onehot_dequant"] = bits(f.dequantize())
    np.savez_compressed(os.path.join(HERE, "wo8.npz"), **out)
    configs = {
        "Int8WeightOnlyConfig": config_to_dict(Int8WeightOnlyConfig()),
        "Float8WeightOnlyConfig": config_to_dict(Float8WeightOnlyConfig()),
        "Int8WeightOnlyConfig_tensor": config_to_dict(Int8WeightOnlyConfig(granularity=PerTensor())),
        "Float8WeightOnlyConfig_tensor": config_to_dict(Float8WeightOnlyConfig(granularity=PerTensor())),
    }
    with open(os.path.join(HERE, "wo8_configs.json"), "w") as fh:
        json.dump(configs, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print({k: v.shape for k, v in out.items()})
    print(json.dumps(configs))


if __name__ == "__main__":
    main()
