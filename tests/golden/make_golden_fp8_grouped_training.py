"""Generate tests/golden/fp8_grouped_training.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_fp8_grouped_training.py

Everything runs on the CPU.  bf16 tensors are stored as uint16 bit patterns, e4m3 codes as uint8, scales as float32.

  a [256, 128], w [3, 128, 128], go [256, 128]   the operands (seed 0: randn, W * 0.05, go * 0.01): M = 256, E = 3, N = K = 128;
                     B_t = w.transpose(-2, -1), the column-major [E, K, N] view the reference takes
  offs [3]           48, 208, 256: the middle group starts and ends inside a 128-token step and spans the boundary at 128
  The six casts of _Float8GroupedMM (torchao/prototype/moe_training/fp8_grouped_mm.py:65-319), all with round_scales_to_power_of_2=True,
  by the torch code the reference tests its Triton kernels against (the kernels themselves do not run here):
  a_r_q/_s, go_r_q/_s    tensor_to_scale(t, AXISWISE, axiswise_dim=-1) + to_fp8_saturated: codes [M, C], scale [M, 1]
  bt_c_q/_s              the same on B_t with axiswise_dim=-2: codes [E, K, N], scale [E, 1, N]
  w3_q/_s                torch_to_3d_rowwise_float8_transpose_rhs(B_t) (utils.py:156-189): codes [E, N, K] (a column-major view, stored
                         here as the contiguous [E, K, N] behind it), scale [E, 1, K]
  go_j_q/_s, a_j_q/_s    torch_to_float8_per_group_colwise(t, offs) (utils.py:20-86): codes [M, C], scale [E * C]
  out [M, N], grad_a [M, K], grad_w [E, N, K]   the three GEMMs on the dequantised casts, per group in float64, rounded once to bf16
                         (the reference's own Function needs Triton and torch._scaled_grouped_mm: this composition is its emulation);
                         grad_B_t is grad_w.transpose(-2, -1)

The recorder asserts that every scale is a power of two and every code finite.  The per-group helper raises on an empty group and leaves
rows past the last offset unwritten: the fixture has neither.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fp8_grouped_training.npz")
M, E, N, K = 256, 3, 128, 128
OFFS = (48, 208, 256)


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def load(path=PATH):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def to_bf16_bits(x64):
    """float64 -> bf16 bits, ONE rounding (round to nearest, ties to even)."""
    x64 = np.ascontiguousarray(x64, dtype=np.float64)
    u = x64.view(np.uint64)
    # bf16 keeps 7 mantissa bits: drop 45 of float64's 52 (every value here is a normal bf16: no exponent handling is needed)
    lsb = (u >> np.uint64(45)) & np.uint64(1)
    r = (u + np.uint64((1 << 44) - 1) + lsb) >> np.uint64(45) << np.uint64(45)
    y = r.view(np.float64).astype(np.float32)  # exact: 8 significant bits
    assert np.all((y.view(np.uint32) & 0xFFFF) == 0) and np.all(np.isfinite(y)) and np.all((np.abs(y) > 1e-30) | (y == 0))
    return (y.view(np.uint32) >> 16).astype(np.uint16)


def sqnr(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(10 * np.log10((ref ** 2).sum() / ((x - ref) ** 2).sum()))


def main():
    from torchao.float8.config import ScalingGranularity
    from torchao.float8.float8_utils import tensor_to_scale, to_fp8_saturated
    from torchao.prototype.moe_training.utils import torch_to_3d_rowwise_float8_transpose_rhs, torch_to_float8_per_group_colwise

    f8 = torch.float8_e4m3fn
    g = torch.Generator().manual_seed(0)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(E, N, K, generator=g) * 0.05).to(torch.bfloat16)
    go = (torch.randn(M, N, generator=g) * 0.01).to(torch.bfloat16)
    offs = torch.tensor(OFFS, dtype=torch.int32)
    b_t = w.transpose(-2, -1)
    out = {"a": bits(a), "w": bits(w), "go": bits(go), "offs": offs.numpy().copy()}

    def rec(key, q, s):
        q, s = q.contiguous().view(torch.uint8).numpy().copy(), s.to(torch.float32).contiguous().numpy().copy()
        assert not np.any((q & 0x7F) == 0x7F), "a non-finite code"
        assert np.all((s.view(np.uint32) & 0x7FFFFF) == 0) and np.all(s > 0), "a scale that is no power of two"
        out[key + "_q"], out[key + "_s"] = q, s
        return torch.from_numpy(q).view(f8).to(torch.float64), torch.from_numpy(s).to(torch.float64)

    def axiswise(t, dim):
        s = tensor_to_scale(t, f8, scaling_granularity=ScalingGranularity.AXISWISE, axiswise_dim=dim, round_scales_to_power_of_2=True)
        return to_fp8_saturated(t.to(torch.float32) * s, f8), s

    a_q, a_s = rec("a_r", *axiswise(a, -1))
    go_q, go_s = rec("go_r", *axiswise(go, -1))
    bt_q, bt_s = rec("bt_c", *axiswise(b_t, -2))
    w3_qv, w3_sv = torch_to_3d_rowwise_float8_transpose_rhs(b_t, f8, round_scales_to_power_of_2=True)
    assert tuple(w3_qv.shape) == (E, N, K) and tuple(w3_sv.shape) == (E, 1, K) and w3_qv.transpose(-2, -1).is_contiguous()
    w3_q, w3_s = rec("w3", w3_qv.transpose(-2, -1), w3_sv)  # [E, K, N] codes, scale per (e, k)
    goj_q, goj_s = rec("go_j", *torch_to_float8_per_group_colwise(go, offs, f8, round_scales_to_power_of_2=True))
    aj_q, aj_s = rec("a_j", *torch_to_float8_per_group_colwise(a, offs, f8, round_scales_to_power_of_2=True))

    dq_a, dq_go = a_q / a_s, go_q / go_s                    # [M, K], [M, N]
    dq_bt = bt_q / bt_s                                     # [E, K, N]
    dq_w3 = w3_q / w3_s.transpose(-2, -1)                   # [E, K, N] / [E, K, 1]
    y = torch.zeros(M, N, dtype=torch.float64)
    ga = torch.zeros(M, K, dtype=torch.float64)
    gw = torch.zeros(E, N, K, dtype=torch.float64)
    lo = 0
    for e, hi in enumerate(OFFS):
        y[lo:hi] = dq_a[lo:hi] @ dq_bt[e]
        ga[lo:hi] = dq_go[lo:hi] @ dq_w3[e].t()
        dg = goj_q[lo:hi] / goj_s[e * N:(e + 1) * N]
        dx = aj_q[lo:hi] / aj_s[e * K:(e + 1) * K]
        gw[e] = dg.t() @ dx
        lo = hi
    out["out"], out["grad_a"], out["grad_w"] = to_bf16_bits(y.numpy()), to_bf16_bits(ga.numpy()), to_bf16_bits(gw.numpy())

    a32, w32, go32 = a.float(), w.float(), go.float()
    y32, ga32, gw32 = torch.zeros(M, N), torch.zeros(M, K), torch.zeros(E, N, K)
    lo = 0
    for e, hi in enumerate(OFFS):
        y32[lo:hi], ga32[lo:hi], gw32[e] = a32[lo:hi] @ w32[e].t(), go32[lo:hi] @ w32[e], go32[lo:hi].t() @ a32[lo:hi]
        lo = hi
    print("SQNR vs fp32 matmuls: out %.2f dB, grad_A %.2f dB, grad_B %.2f dB" % (
        sqnr(y.numpy(), y32.numpy()), sqnr(ga.numpy(), ga32.numpy()), sqnr(gw.numpy(), gw32.numpy())))
    np.savez_compressed(PATH, **out)
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
