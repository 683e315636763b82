"""Generate tests/golden/intx.npz by importing the REFERENCE (torchao) on the CPU.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_intx.py

bf16 tensors are stored as uint16 bit patterns; the archive is compressed.

  w [24, 256]            the weight.  Planted: row 0 group 0 (of 32) all zero, row 1 all zero; row 2 group 0 all 0.75, row 3 all -1.5
                         (all-equal and negative-only at every group size); row 4 negative only; row 5 halves up to 127.5 and row 6 halves up
                         to 7.5 (ties at .5 under the int8 / int4 symmetric scales, which are 1); row 7 bf16 subnormals and row 8 +-2^-125
                         (the scale clamps to eps); row 9 values at 2^-20 with some at 2^6
  b{b}_{mapping}_g{g}_q / _s / _zp / _dq   IntxUnpackedToInt8Tensor.from_hp(w, (1, g), torch.int{b}, mapping_type=mapping) -> qdata, scale,
                         zero_point, and its dequantize(); b in 1..8, the three mappings, g in {32, 128, 256}
  x [6, 256], x_fq       an activation (row 1 constant, row 2 zeros, row 3 negative only) and _apply_int8_act_asym_per_token_quant_dequant(x)
The maker asserts that tests/intx_ref.py reproduces every recorded byte."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import intx_ref  # noqa: E402

from torchao.quantization.quant_primitives import MappingType  # noqa: E402
from torchao.quantization.quantize_.workflows.intx.intx_unpacked_to_int8_tensor import (  # noqa: E402
    IntxUnpackedToInt8Tensor,
    _apply_int8_act_asym_per_token_quant_dequant,
)

GROUPS = (32, 128, 256)


def bits(t):
    """bf16 -> uint16 bit patterns, every NaN as 0x7FC0 (the CPU's conversions give 0xFFFF from vector loops and 0x7FC0 from scalar tails)"""
    b = t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()
    b[torch.isnan(t).numpy()] = intx_ref.NAN_BITS
    return b


def weight():
    gen = torch.Generator().manual_seed(0)
    w = torch.randn(24, 256, generator=gen).to(torch.bfloat16)
    w[0, :32] = 0.0
    w[1] = 0.0
    w[2, :32] = 0.75
    w[3] = -1.5
    w[4] = -w[4].abs() - 0.0078125
    halves = (torch.arange(256) % 32).float() - 15.5
    w[5] = (halves * 4).to(torch.bfloat16)
    w[5, 0], w[5, 1] = 127.5, -127.5
    w[6] = (halves / 4).round().add(0.5).to(torch.bfloat16)
    w[6, 0::32], w[6, 1::32] = 7.5, -7.5
    w[7] = (torch.randn(256, generator=gen) * 2.0 ** -130).to(torch.bfloat16)
    w[8] = torch.where(torch.arange(256) % 2 == 0, 2.0 ** -125, -(2.0 ** -125)).to(torch.bfloat16)
    w[9] = (torch.randn(256, generator=gen) * 2.0 ** -20).to(torch.bfloat16)
    w[9, 5::37] = 64.0
    return w


def main():
    w = weight()
    out = {"w": bits(w)}
    for b in range(1, 9):
        for mapping in intx_ref.MAPPINGS:
            for g in GROUPS:
                t = IntxUnpackedToInt8Tensor.from_hp(w, (1, g), getattr(torch, f"int{b}"), mapping_type=MappingType[mapping])
                key = f"b{b}_{mapping}_g{g}"
                out[key + "_q"], out[key + "_s"], out[key + "_zp"] = t.qdata.numpy(), bits(t.scale), t.zero_point.numpy()
                out[key + "_dq"] = bits(t.dequantize())
                q, s, zp = intx_ref.from_hp(out["w"], b, mapping, g)
                for name, got in (("q", q), ("s", s), ("zp", zp), ("dq", intx_ref.dequantize(q, s, zp))):
                    bad = np.argwhere(got != out[f"{key}_{name}"])
                    assert bad.size == 0, f"{key}_{name}: restatement differs at {bad[:4].tolist()}: {got[tuple(bad[0])]} vs {out[f'{key}_{name}'][tuple(bad[0])]}"
    gen = torch.Generator().manual_seed(1)
    x = (torch.randn(6, 256, generator=gen) * 3).to(torch.bfloat16)
    x[1], x[2], x[3] = 0.3125, 0.0, -x[3].abs() - 1
    out["x"], out["x_fq"] = bits(x), bits(_apply_int8_act_asym_per_token_quant_dequant(x))
    assert np.array_equal(intx_ref.act_fake_quant(out["x"]), out["x_fq"])
    path = os.path.join(HERE, "intx.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
