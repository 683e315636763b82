"""Generate tests/golden/blockwise_fp8_training.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the
file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_blockwise_fp8_training.py

Everything runs on the CPU, from the reference's torch functions (prototype/blockwise_fp8_training/kernels.py:1031-1156), which are the
contract of the casts.  bf16 tensors are stored as uint16 bit patterns, e4m3 codes as uint8, reciprocal scales as float32.

  x [2, 128, 256], w [128, 256], go [2, 128, 128]   the operands (randn, W * 0.05, go * 0.01): M = 256, N = 128, K = 256
  edge [256, 256]    rows scaled by 2^-12 .. 2^12; a zero 1 x 128 block (row 3, columns 0..127) and one that holds only 1e-20 (row 4); a
                     zero 128 x 1 block (column 5, rows 128..255) and one that holds only 1e-20 (column 6); a zero 128 x 128 block (rows
                     128.., columns 128..); the largest finite bf16 at [7, 139]; block maxima in a block's last row and last column
                     ([127, 127] and [255, 127])
  <t>_row_q, _row_inv   torch_blockwise_scale_act_quant_lhs(t):  codes [R, C], reciprocal scales [R, C/128]      t in x, go, edge
  <t>_col_q, _col_inv   torch_blockwise_scale_act_quant_rhs(t):  codes [R, C] (the function's logical layout; the HIP cast stores them
                        transposed), reciprocal scales [R/128, C]                                                 t in x, go, edge
  <t>_blk_q, _blk_inv   torch_blockwise_scale_weight_quant(t):   codes [N, K], reciprocal scales [N/128, K/128]   t in w, edge

The recorder asserts that all codes are finite, that cast(w.t()) has the transposed codes and scales of cast(w), and that at least one
recorded element has |f32(x) * scale| > 448 before the clamp (the clamp is live); where the random data gives none it searches for a
bf16 amax that does and plants it in x.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "blockwise_fp8_training.npz")
B, T, N, K = 2, 128, 128, 256
ROW, COL, BLK = ("x", "go", "edge"), ("x", "go", "edge"), ("w", "edge")


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def load(path=PATH):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def edge_tensor():
    g = torch.Generator().manual_seed(1)
    e = torch.randn(256, 256, generator=g) * torch.exp2((torch.arange(256) % 25 - 12).float())[:, None]
    e[3, :128] = 0.0
    e[4, :128] = 0.0
    e[4, 64] = 1e-20
    e[128:, 5] = 0.0
    e[128:, 6] = 0.0
    e[200, 6] = 1e-20
    e[128:, 128:] = 0.0
    e[7, 139] = torch.finfo(torch.bfloat16).max
    e[127, 127] = -3.0e5
    e[255, 127] = 2.0e5
    return e.to(torch.bfloat16)


def overshoots(t, scale):
    """How many elements of bf16 t have |f32(t) * scale| > 448 before the clamp (scale expanded to t's shape)."""
    return int((t.float() * scale).abs().gt(448.0).sum())


def row_scale(t):
    """The 1 x 128 scales of t as torch_blockwise_scale_act_quant_lhs computes them, one per element."""
    amax = t.reshape(-1, 128).abs().max(dim=1, keepdim=True).values.to(torch.float64).clamp(min=1e-12)
    return (448.0 / amax).to(torch.float32).reshape(t.shape[0], -1).repeat_interleave(128, dim=1)


def plant_overshoot(x):
    """A bf16 amax a with f32(a) * f32(448 / a) > 448, placed at x[0, 0, 0] as its blocks' maximum."""
    for b in range(0x4100, 0x4180):  # bf16 values in [8, 16): above every |randn| drawn here
        a = torch.tensor([b], dtype=torch.int16).view(torch.bfloat16)
        s = (448.0 / a.to(torch.float64)).to(torch.float32)
        if float((a.float() * s).item()) > 448.0:
            x[0, 0, 0] = a[0]
            return float(a.item())
    raise AssertionError("no bf16 amax in [8, 16) overshoots 448")


def main():
    from torchao.prototype.blockwise_fp8_training.kernels import (
        torch_blockwise_scale_act_quant_lhs,
        torch_blockwise_scale_act_quant_rhs,
        torch_blockwise_scale_weight_quant,
    )

    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    go = (torch.randn(B, T, N, generator=g) * 0.01).to(torch.bfloat16)
    edge = edge_tensor()
    tensors = {"x": x.reshape(-1, K), "go": go.reshape(-1, N), "w": w, "edge": edge}
    if not any(overshoots(t, row_scale(t)) for t in (tensors["x"], tensors["go"], edge)):
        print("no element overshoots 448 in the random data: planted %r in x" % plant_overshoot(x))
        tensors["x"] = x.reshape(-1, K)
    n_over = sum(overshoots(t, row_scale(t)) for t in (tensors["x"], tensors["go"], edge))
    assert n_over > 0, "the clamp is not exercised"
    print("%d recorded elements have |f32(x) * scale| > 448 before the clamp (1 x 128 casts)" % n_over)

    out = {"x": bits(x), "w": bits(w), "go": bits(go), "edge": bits(edge)}

    def record(key, q, inv, shape):
        q, inv = q.contiguous().view(torch.uint8).numpy().copy(), inv.contiguous().to(torch.float32).numpy().copy()
        assert q.shape == tuple(shape) and not np.any((q & 0x7F) == 0x7F), "a non-finite code in " + key
        assert np.all(np.isfinite(inv)) and np.all(inv > 0), "a non-finite reciprocal in " + key
        out[key + "_q"], out[key + "_inv"] = q, inv

    for name in ROW:
        t = tensors[name]
        record(name + "_row", *torch_blockwise_scale_act_quant_lhs(t.contiguous()), t.shape)
    for name in COL:
        t = tensors[name]
        record(name + "_col", *torch_blockwise_scale_act_quant_rhs(t.contiguous()), t.shape)
    for name in BLK:
        t = tensors[name]
        record(name + "_blk", *torch_blockwise_scale_weight_quant(t.contiguous()), t.shape)
        qt, invt = torch_blockwise_scale_weight_quant(t.t().contiguous())
        assert np.array_equal(qt.view(torch.uint8).numpy(), out[name + "_blk_q"].T), "cast(w.t()) is not the transpose of cast(w)"
        assert np.array_equal(invt.numpy(), out[name + "_blk_inv"].T)

    # the edge cases are what they are meant to be
    zero = np.float32(1.0) / np.float32(448.0 / 1e-12)
    assert out["edge_row_inv"][3, 0] == zero and out["edge_row_inv"][4, 0] == zero and not out["edge_row_q"][3:5, :128].any()
    assert out["edge_blk_inv"][1, 1] == zero and not out["edge_blk_q"][128:, 128:].any()
    assert not out["edge_col_q"][128:, 5:7].any()
    print("a zero 128 x 1 block: reciprocal %r (1 x 128 and 128 x 128: %r)" % (float(out["edge_col_inv"][1, 5]), float(zero)))
    assert out["edge_row_q"][7, 139] == 0x7E  # the largest bf16 lands on 448

    np.savez_compressed(PATH, **out)
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
