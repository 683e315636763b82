"""Generate tests/golden/nf4.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_nf4.py

Everything runs on the CPU in bf16: to_nf4 (NF4Tensor.from_tensor), get_original_weight, linear_nf4 forward and backward.  bf16 tensors
are stored as uint16 bit patterns.  Per case <c>: <c>_x the weight, <c>_meta = (rows, cols, block_size, scaler_block_size), the five
fields <c>_codes / _scalers / _factors / _mean (and <c>_absmax, get_block_absmax), <c>_w the dequantized weight, <c>_m0 the scaler blocks
whose centred scalers are all zero (the reference's NaN -> int8 there is undefined behaviour: recorded, never compared), and for the cases
that hold no NaN <c>_in / _go / _y / _gi: an activation, a grad_output, linear_nf4's forward and its grad_input.

  b64         [64, 256]  at (64, 256): one scaler block
  two         [128, 256] at (64, 256): two scaler blocks
  straddle    [512, 96]  at (64, 256): blocks straddle rows
  sb8a, sb8b  [17, 512] and [40, 128] at (64, 8)
  b32, b128   [32, 128] at (32, 8) and [32, 256] at (128, 8)
  planted     [24, 64] at (64, 1): an all-zero block (0 / 0: NaN -> code 0), an all-equal block, a block holding the largest bf16 (its
              factor is 0 and its scaler NaN), bf16 subnormals, a +- tie for the block maximum
  m0          [32, 64] at (64, 16): the second scaler block's maxima all equal the mean, m = 0
  exact       [64, 256] at (64, 256): block maxima that are multiples of 2^-8 and <= 1 -- every partial sum of the mean is exact in fp32,
              so the mean is the same bits in any summation order
  code_table  quantize_tensor_nearest over ALL 65536 bf16 patterns

The maker asserts that tests/nf4_ref.py reproduces every recorded byte (NaN results compared as NaN: their sign and payload are the
processor's).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nf4_ref as R  # noqa: E402

from torchao.quantization.quantize_.workflows.nf4.nf4_tensor import NF4Tensor, get_block_absmax, linear_nf4, to_nf4  # noqa: E402


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def from_bits(b, shape):
    return torch.from_numpy(np.asarray(b, dtype=np.uint16).view(np.int16).copy()).view(torch.bfloat16).reshape(shape)


def gaussian(shape, seed, spread=True):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g) * 0.05
    if spread:  # rows of different magnitude, so that the centred scalers use the int8 range
        w = w * torch.exp(torch.randn(shape[0], 1, generator=g))
    return w.to(torch.bfloat16)


def planted():
    g = torch.Generator().manual_seed(77)
    w = (torch.randn(24, 64, generator=g) * 0.3).to(torch.bfloat16)
    w[0] = 0.0                                                     # 0 / 0
    w[1] = 0.37109375                                              # all equal: every v = 1
    w[2, 5] = torch.finfo(torch.bfloat16).max                      # the largest bf16
    sub = torch.tensor([1, 2, 3, 0x7F, 0x40, 0x8001, 0x807F, 0x20, 0, 0x8000, 5, 0x8005, 0x11, 0x33, 0x55, 0x77] * 4, dtype=torch.int32)
    w[3] = sub.to(torch.int16).view(torch.bfloat16)                # bf16 subnormals only
    w[4] = (torch.randn(64, generator=g) * 0.2).to(torch.bfloat16)
    w[4, 7], w[4, 40] = 1.5, -1.5                                  # a +- tie for the maximum
    w[5, :32] = sub[:32].to(torch.int16).view(torch.bfloat16)      # subnormals under a normal maximum
    return w


def m0_case():
    g = torch.Generator().manual_seed(78)
    w = (torch.rand(32, 64, generator=g) * 0.4 - 0.2).to(torch.bfloat16)
    for b in range(16):
        w[b, (b * 7) % 64] = 0.5 if b % 2 else -1.5                # first scaler block: maxima 0.5 / 1.5, mean 1
    for b in range(16, 32):
        w[b, (b * 5) % 64] = 1.0 if b % 3 else -1.0                # second: every maximum equals the mean
    return w


def exact_mean_case():
    g = torch.Generator().manual_seed(79)
    w = torch.randn(64, 256, generator=g)
    blocks = w.view(-1, 64)
    k = torch.randint(1, 257, (blocks.shape[0], 1), generator=g).float() / 256.0
    blocks = blocks / blocks.abs().amax(dim=1, keepdim=True) * k * 0.98
    blocks[torch.arange(blocks.shape[0]), torch.randint(0, 64, (blocks.shape[0],), generator=g)] = k[:, 0] * torch.where(
        torch.rand(blocks.shape[0], generator=g) < 0.5, -1.0, 1.0)
    return blocks.reshape(64, 256).to(torch.bfloat16)


def same(a, b, nan_a=None):
    """equal bits, or NaN in both (a, b uint16 bf16 bits)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint16:
        return bool(np.array_equal(a, b))
    isnan = lambda v: (v & 0x7FFF) > 0x7F80  # noqa: E731
    return bool(np.all((a == b) | (isnan(a) & isnan(b))))


def record(out, name, w, B, SB, with_linear=True):
    t = to_nf4(w, B, SB)
    rec = {
        "x": bits(w), "meta": np.array([w.shape[0], w.shape[1], B, SB], dtype=np.int64),
        "absmax": bits(get_block_absmax(w.flatten(), B)),
        "codes": t.quantized_data.numpy().copy(), "scalers": t.quantized_scalers.numpy().copy(),
        "factors": bits(t.quantization_factor), "mean": bits(t.scaler_mean.reshape(1)),
        "w": bits(t.get_original_weight()),
    }
    assert t.quantized_data.dtype == torch.uint8 and t.quantized_scalers.dtype == torch.int8
    assert t.quantization_factor.dtype == torch.bfloat16 and t.scaler_mean.dtype == torch.bfloat16
    # the restatement gives the reference's bytes
    absmax, codes, q, qf, m0 = R.quantize(rec["x"], B, SB, rec["mean"])
    rec["m0"] = m0
    keep = ~np.repeat(m0, SB)
    assert same(absmax, rec["absmax"]), name
    assert same(codes, rec["codes"]), name
    assert same(qf, rec["factors"]), name
    assert same(q[keep], rec["scalers"][keep]), name
    assert same(R.dequantize(rec["codes"], rec["scalers"], rec["factors"], rec["mean"], B, SB), rec["w"].reshape(-1)), name
    if with_linear:
        g = torch.Generator().manual_seed(len(name) + w.shape[0])
        x = torch.randn(5, w.shape[1], generator=g).to(torch.bfloat16).requires_grad_(True)
        go = torch.randn(5, w.shape[0], generator=g).to(torch.bfloat16)
        y = linear_nf4(x, t)
        y.backward(go)
        rec.update({"in": bits(x.detach()), "go": bits(go), "y": bits(y.detach()), "gi": bits(x.grad)})
    for k, v in rec.items():
        out[f"{name}_{k}"] = v
    print(name, tuple(w.shape), B, SB, "m0 blocks:", int(m0.sum()), "codes used:", len(set(R.unpack(rec["codes"]).tolist())))


def main():
    out = {}
    record(out, "b64", gaussian((64, 256), 1), 64, 256)
    record(out, "two", gaussian((128, 256), 2), 64, 256)
    record(out, "straddle", gaussian((512, 96), 3), 64, 256)
    record(out, "sb8a", gaussian((17, 512), 4), 64, 8)
    record(out, "sb8b", gaussian((40, 128), 5), 64, 8)
    record(out, "b32", gaussian((32, 128), 6), 32, 8)
    record(out, "b128", gaussian((32, 256), 7), 128, 8)
    record(out, "planted", planted(), 64, 1, with_linear=False)
    record(out, "m0", m0_case(), 64, 16)
    assert out["m0_m0"].tolist() == [False, True], out["m0_m0"]
    record(out, "exact", exact_mean_case(), 64, 256)
    a = R.bf16.from_bits(out["exact_absmax"]).astype(np.float64) * 256
    assert np.all(a == np.round(a)) and a.max() <= 256 and a.min() >= 1
    # the code rule over every bf16 pattern
    allv = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    nf4 = torch.tensor(R.TABLE, dtype=torch.bfloat16)
    table = NF4Tensor.quantize_tensor_nearest(allv, nf4).to(torch.uint8).numpy()
    assert np.array_equal(R.codes_of(R.bf16.from_bits(np.arange(65536, dtype=np.uint16))), table)
    assert np.array_equal(R.bf16.to_bits(R.TABLE_BF16), bits(nf4)) and R.table_is_on_the_2_pow_minus_11_grid()
    out["code_table"] = table
    path = os.path.join(HERE, "nf4.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
