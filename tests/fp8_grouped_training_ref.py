"""numpy restatement of the casts and GEMMs of the float8 rowwise MoE grouped GEMM's training step (torchao/prototype/moe_training/
fp8_grouped_mm.py:65-319).  TEST INFRASTRUCTURE ONLY, built on tests/fp8_training_ref.py (the scale and cast arithmetic).  Pinned against
tests/golden/fp8_grouped_training.npz, which tests/golden/make_golden_fp8_grouped_training.py writes from the reference on the CPU.

  group_colwise  utils.py:20-86 (torch_to_float8_per_group_colwise): one scale per column and token group, the amax over the group's rows.
                 Beyond the reference's helper, the rules of include/ao_mi355.h: an empty group gets the scale of a zero amax, rows at or
                 past offs[-1] belong to no group and get code 0.
  colwise_3d     utils.py:156-189 (torch_to_3d_rowwise_float8_transpose_rhs): w [E, R, C] cast along R, per expert.
  rowwise        tensor_to_scale(axiswise_dim=-1) + to_fp8_saturated.
  The GEMMs sum the dequantised operands per group in float64; `to_bf16_bits` rounds a float64 result once.

bf16 tensors are uint16 bit patterns, e4m3 codes uint8, scales float32.
"""
import numpy as np

import fp8_training_ref as T
from fp8_training_ref import bf16, fp8_ref  # noqa: F401


def rowwise(xb, pow2=True):
    """x bf16 [R, C] -> (codes [R, C], scale [R, 1], inv_scale [R, 1])."""
    return T.cast(xb, -1, pow2)


def group_colwise(xb, offs, pow2=True):
    """x bf16 [R, C], offs [E] cumulative ends -> (codes [R, C] in x's own layout, scale [E, C], inv_scale [E, C])."""
    xb = np.asarray(xb, dtype=np.uint16)
    r, c = xb.shape
    q = np.zeros((r, c), dtype=np.uint8)
    s = np.empty((len(offs), c), dtype=np.float32)
    lo = 0
    for e, hi in enumerate(int(o) for o in offs):
        if hi > lo:
            q[lo:hi], se, _ = T.cast(xb[lo:hi], 0, pow2)
            s[e] = se[0]
        else:
            s[e] = T.amax_to_scale(np.zeros(c, dtype=np.float32), pow2)
        lo = max(lo, hi)
    return q, s, (np.float32(1.0) / s).astype(np.float32)


def colwise_3d(wb, pow2=True):
    """w bf16 [E, R, C] -> (codes [E, R, C] in w's own layout, scale [E, C], inv_scale [E, C]); the amax along R."""
    wb = np.asarray(wb, dtype=np.uint16)
    q = np.empty(wb.shape, dtype=np.uint8)
    s = np.empty((wb.shape[0], wb.shape[2]), dtype=np.float32)
    for e in range(wb.shape[0]):
        q[e], se, _ = T.cast(wb[e], 0, pow2)
        s[e] = se[0]
    return q, s, (np.float32(1.0) / s).astype(np.float32)


def to_bf16_bits(x64):
    """float64 -> bf16 bits by ONE rounding to nearest, ties to even (normal results only)."""
    x64 = np.ascontiguousarray(x64, dtype=np.float64)
    u = x64.view(np.uint64)
    lsb = (u >> np.uint64(45)) & np.uint64(1)
    r = (u + np.uint64((1 << 44) - 1) + lsb) >> np.uint64(45) << np.uint64(45)
    y = r.view(np.float64).astype(np.float32)
    assert np.all((y.view(np.uint32) & 0xFFFF) == 0) and np.all(np.isfinite(y)) and np.all((np.abs(y) > 1e-30) | (y == 0))
    return (y.view(np.uint32) >> 16).astype(np.uint16)


def _groups(offs, m):
    lo = 0
    for e, hi in enumerate(int(o) for o in offs):
        hi = min(max(hi, 0), m)
        yield e, lo, max(lo, hi)
        lo = max(lo, hi)


def grouped_mm(a_q, a_s, b_q, b_s, offs):
    """a codes [M, K], a_s [M, 1]; b codes [E, N, K], b_s [E, N] (one scale per (e, n)); -> float64 [M, N], rows past offs[-1] zero."""
    a = T.dequant(a_q, a_s)
    y = np.zeros((a_q.shape[0], b_q.shape[1]), dtype=np.float64)
    for e, lo, hi in _groups(offs, a_q.shape[0]):
        y[lo:hi] = a[lo:hi] @ T.dequant(b_q[e], np.asarray(b_s[e]).reshape(-1, 1)).T
    return y


def wgrad(g_q, g_s, x_q, x_s, offs, with_mag=False):
    """g codes [M, N], g_s [E, N]; x codes [M, K], x_s [E, K] (the jagged casts) -> float64 [E, N, K]; with_mag: also sum |g| |x|."""
    e_n = len(offs)
    out = np.zeros((e_n, g_q.shape[1], x_q.shape[1]), dtype=np.float64)
    mag = np.zeros_like(out)
    for e, lo, hi in _groups(offs, g_q.shape[0]):
        g, x = T.dequant(g_q[lo:hi], g_s[e][None, :]), T.dequant(x_q[lo:hi], x_s[e][None, :])
        out[e], mag[e] = g.T @ x, np.abs(g).T @ np.abs(x)
    return (out, mag) if with_mag else out
