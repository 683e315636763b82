"""Generate tests/golden/fp8_block_grouped.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_fp8_block_grouped.py

Everything runs on the CPU.  Two cases of the blockwise float8 grouped GEMM (token groups against experts):
  A: group sizes [129, 0, 71], N = 256, K = 256        B: group sizes [2, 0, 5, 1], N = 128, K = 256
Per case <c>: the bf16 activation bits <c>_x (seeded, rows spread over 2^[-3, 3]), its codes and scales <c>_aq / <c>_as from
Float8Tensor.from_hp(x, granularity=PerBlock([1, 128])), the per-expert weight codes and scales <c>_wq [E, N, K] / <c>_ws
[E, N/128, K/128] from PerBlock([128, 128]) on weights randn * 0.05 (weights(seed, E, N, K) below: the host test draws them again
rather than storing them), <c>_offs, and <c>_emulated: the bf16 bits of the reference's CPU-runnable backend,
_emulated_blockwise_scaled_grouped_mm_impl (prototype/blockwise_fp8_training/grouped_kernels.py:78-93: both operands dequantized to
bf16, then torch._grouped_mm), on those codes and scales.  bf16 tensors are stored as uint16 bit patterns, e4m3 codes as uint8, scales
as float32.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"A": ([129, 0, 71], 256, 256, 11), "B": ([2, 0, 5, 1], 128, 256, 12)}  # sizes, N, K, seed


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def weights(seed, E, N, K):
    """bf16 [E, N, K], the first draw of the case's generator."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(E, N, K, generator=g) * 0.05).to(torch.bfloat16), g


def main():
    from torchao.prototype.blockwise_fp8_training.grouped_kernels import _emulated_blockwise_scaled_grouped_mm_impl
    from torchao.prototype.blockwise_fp8_training.kernels import BLOCKWISE_1X128_SCALING_TYPE, BLOCKWISE_128X128_SCALING_TYPE
    from torchao.quantization import PerBlock
    from torchao.quantization.quantize_.workflows.float8.float8_tensor import Float8Tensor

    out = {}
    for name, (sizes, N, K, seed) in CASES.items():
        E, M = len(sizes), sum(sizes)
        w, g = weights(seed, E, N, K)
        x = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).to(torch.bfloat16)
        offs = torch.tensor(np.cumsum(sizes), dtype=torch.int32)
        xt = Float8Tensor.from_hp(x, granularity=PerBlock([1, 128]))
        wts = [Float8Tensor.from_hp(w[e], granularity=PerBlock([128, 128])) for e in range(E)]
        aq, a_s = xt.qdata, xt.scale.to(torch.float32)
        wq, ws = torch.stack([t.qdata for t in wts]), torch.stack([t.scale.to(torch.float32) for t in wts])
        assert tuple(a_s.shape) == (M, K // 128) and tuple(ws.shape) == (E, N // 128, K // 128)
        # the reference's operand layout: b the column-major [E, K, N] view, its scales [E, K/128, N/128]
        emu = _emulated_blockwise_scaled_grouped_mm_impl(aq, wq.transpose(-2, -1), a_s, BLOCKWISE_1X128_SCALING_TYPE, ws.transpose(-2, -1),
                                                         BLOCKWISE_128X128_SCALING_TYPE, offs, torch.bfloat16, 128)
        assert tuple(emu.shape) == (M, N) and emu.dtype == torch.bfloat16
        out[f"{name}_x"], out[f"{name}_aq"], out[f"{name}_as"] = bits(x), aq.view(torch.uint8).numpy().copy(), a_s.numpy().copy()
        out[f"{name}_wq"], out[f"{name}_ws"] = wq.view(torch.uint8).numpy().copy(), ws.numpy().copy()
        out[f"{name}_offs"], out[f"{name}_emulated"] = offs.numpy().copy(), bits(emu)
    path = os.path.join(HERE, "fp8_block_grouped.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
