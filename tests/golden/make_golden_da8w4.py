"""Generate tests/golden/da8w4.npz from the REFERENCE (torchao) on the CPU; run once, commit the file:
    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_da8w4.py
Its choose_qparams_affine / quantize_affine with the arguments of from_hp_da8w4 (weight) and _da8w4_linear (activation, both mappings); bf16 as
uint16 bits.  w [32, 384], planted per group of 32: rows 0 / 1 zero, 2 / 3 all-equal, 4 positive only (zp 0), 5 negative only (zp 15), 6 halves
in -8 .. 7 (scale 1: .5 ties), 7 at 2^-24 (eps clamp); recorded on w[:, :K], K in {g, 3 g}.  x [6, 384]: row 1 constant, 2 zero, 3 negative
only, 4 halves in -128 .. 127 (ties), 5 at 2^-30 (eps); recorded on x[:, :K], K in {32, 384}.  Asserts that tests/da8w4_ref.py gives every byte."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import da8w4_ref as R  # noqa: E402

from torchao.quantization.quant_primitives import MappingType, choose_qparams_affine, quantize_affine  # noqa: E402


def tensors():
    gen = torch.Generator().manual_seed(0)
    w = torch.randn(32, 384, generator=gen).to(torch.bfloat16)
    w[0, :32] = 0.0
    w[1] = 0.0
    w[2, :32] = 0.75
    w[3] = -1.5
    w[4] = w[4].abs() + 0.0078125
    w[5] = -w[5].abs() - 0.0078125
    w[6] = ((torch.arange(384) % 16).float() - 8.0 + 0.5).to(torch.bfloat16)
    w[6, 0::32], w[6, 1::32] = -8.0, 7.0
    w[7] = (torch.randn(384, generator=gen) * 2.0 ** -24).to(torch.bfloat16)
    gen = torch.Generator().manual_seed(1)
    x = (torch.randn(6, 384, generator=gen) * 3).to(torch.bfloat16)
    x[1], x[2], x[3] = 0.3125, 0.0, -x[3].abs() - 1
    x[4] = ((torch.arange(384) % 256).float() - 128.0 + 0.5).to(torch.bfloat16)
    x[4, 0::32], x[4, 1::32] = -128.0, 127.0
    x[5] = (torch.randn(384, generator=gen) * 2.0 ** -30).to(torch.bfloat16)
    return w, x


def record(out, key, t, got, block, mapping, dtype, lo, hi, eps, zdt):
    s, zp = choose_qparams_affine(t, mapping, block, dtype, quant_min=lo, quant_max=hi, eps=eps, scale_dtype=torch.float32, zero_point_dtype=zdt)
    q = quantize_affine(t, block, s, zp, dtype, quant_min=lo, quant_max=hi).to(dtype)
    rec = (q.numpy(), s.reshape(got[1].shape).numpy(), zp.to(torch.int32).reshape(got[2].shape).numpy())
    for name, a, b in zip(("q", "s", "zp"), got, rec):
        assert np.array_equal(a, b), f"{key}_{name}: the restatement differs at {np.argwhere(a != b)[:4].tolist()}"
        out[f"{key}_{name}"] = b


def main():
    w, x = tensors()
    out = {"w": R.bf16.to_bits(w.float().numpy()), "x": R.bf16.to_bits(x.float().numpy())}
    for g in R.GROUPS:
        for k in (g, 3 * g):
            got = R.weight_cast(out["w"][:, :k], g)
            record(out, f"w_g{g}_k{k}", w[:, :k].contiguous(), got, [1, g], MappingType.ASYMMETRIC, torch.uint8, 0, 15, 1e-6, torch.int32)
    eps = torch.finfo(torch.float32).eps
    for k in (32, 384):
        xk = x[:, :k].contiguous()
        record(out, f"x_asym_k{k}", xk, R.act_cast(out["x"][:, :k], False), [1, k], MappingType.ASYMMETRIC, torch.uint8, 0, 255, eps, torch.int32)
        record(out, f"x_sym_k{k}", xk, R.act_cast(out["x"][:, :k], True), [1, k], MappingType.SYMMETRIC, torch.int8, -127, 127, eps, torch.int8)
    np.savez_compressed(os.path.join(HERE, "da8w4.npz"), **out)


if __name__ == "__main__":
    main()
