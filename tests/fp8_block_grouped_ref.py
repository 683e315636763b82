"""numpy restatement of the blockwise float8 grouped GEMM over tests/fp8_block_ref.py: token group e = rows [offs[e-1], offs[e]) of the
activation against expert e, the dense chain per group.  TEST INFRASTRUCTURE ONLY.

The reference has the operation as a training prototype whose CPU-runnable backend dequantizes both operands to bf16 and calls
torch._grouped_mm (torchao/prototype/blockwise_fp8_training/grouped_kernels.py:78-93); tests/golden/fp8_block_grouped.npz records its
output on two cases (tests/golden/make_golden_fp8_block_grouped.py).  The yardsticks of the kernel are the float64 sum and the fp32 chain.

bf16 tensors are uint16 bit patterns, e4m3 codes uint8, scales float32; wq [E, N, K], w_s [E, ceil(N/128), K/128], offs int [E].
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_block_ref as R  # noqa: E402
from oracle import bf16  # noqa: E402  (fp8_block_ref put the repository root on sys.path)


def groups(offs, m_total):
    """[(expert, row_begin, row_end)] of the non-empty groups, with the kernel's reading of offs: bounds clamped to [0, M_total], a
    non-increasing pair is an empty group."""
    out, prev = [], 0
    for e, end in enumerate(np.asarray(offs).tolist()):
        b, t = min(max(prev, 0), m_total), min(max(end, 0), m_total)
        if t > b:
            out.append((e, b, t))
        prev = end
    return out


def offs_of(sizes):
    return np.cumsum(np.asarray(sizes, dtype=np.int64)).astype(np.int32)


def grouped_f64(aq, a_s, wq, w_s, offs):
    """(y, S) float64 [M_total, N]: fp8_block_ref.linear_f64 per non-empty group; rows of no group are zero in both."""
    M, N = aq.shape[0], wq.shape[1]
    y, S = np.zeros((M, N), dtype=np.float64), np.zeros((M, N), dtype=np.float64)
    for e, b, t in groups(offs, M):
        y[b:t], S[b:t] = R.linear_f64(aq[b:t], a_s[b:t], wq[e], w_s[e])
    return y, S


def grouped_chain_bits(aq, a_s, wq, w_s, offs):
    """bf16 bits [M_total, N]: fp8_block_ref.chain_bits per non-empty group; rows of no group are zero."""
    M, N = aq.shape[0], wq.shape[1]
    y = np.zeros((M, N), dtype=np.uint16)
    for e, b, t in groups(offs, M):
        y[b:t] = R.chain_bits(aq[b:t], a_s[b:t], wq[e], w_s[e])
    return y


def cast_experts(wb):
    """w bf16 bits [E, N, K], N and K multiples of 128 -> (codes [E, N, K], scale [E, N/128, K/128]): the 128 x 128 cast per expert."""
    qs = [R.cast_128x128(w) for w in wb]
    return np.stack([q for q, _ in qs]), np.stack([s for _, s in qs])


def l2_to(y64, bits, rows):
    """The l2 distance of a bf16 output (bits) to the float64 result over the first `rows` rows."""
    return float(np.linalg.norm(bf16.from_bits(np.asarray(bits, dtype=np.uint16))[:rows].astype(np.float64) - y64[:rows]))
