"""torch-CPU restatement of the NVFP4 grouped GEMM (ao_nvfp4_grouped_mm): the chains of tests/nvfp4_ref.py per token group against that
group's expert, under that expert's scales.  TEST INFRASTRUCTURE ONLY; pinned against tests/golden/nvfp4_grouped.npz, which
tests/golden/make_golden_nvfp4_grouped.py writes from the reference.  Works on any device.

  group e      rows [offs[e-1], offs[e]) with offs[-1] = 0; rows past offs[E-1] belong to no group (outputs there stay zero here)
  weight-only  R.wo_linear(x[group], b[e], b_s[e], pb[e]): the reference's torch._grouped_mm(x, dequantize(bf16)^T, offs)
  codes        R.mm(a[group], a_s[group], b[e], b_s[e], pa[e], pb[e]): without scales the reference's
               _emulated_nvfp4_scaled_grouped_mm_2d_3d (prototype/moe_training/nvfp4_grouped_mm.py:62-116)
"""
import torch

import nvfp4_ref as R


def offs_of(sizes, device="cpu"):
    """group sizes -> int32 cumulative group ends"""
    return torch.tensor(list(sizes), dtype=torch.int64).cumsum(0).to(torch.int32).to(device)


def groups(offs):
    """(e, begin, end) of every non-empty group"""
    begin = 0
    for e, end in enumerate(offs.tolist()):
        if end > begin:
            yield e, begin, end
        begin = max(begin, end)


def _at(p, e):
    return None if p is None else p.reshape(-1)[e]


def wo_sums(x, b, b_s, offs, pb=None):
    """(m64, S) [M_total, N] of the weight-only chain per group; zero outside the groups"""
    m = torch.zeros(x.shape[0], b.shape[1], dtype=torch.float64, device=x.device)
    S = torch.zeros_like(m)
    for e, r0, r1 in groups(offs):
        m[r0:r1], S[r0:r1] = R.wo_sums(x[r0:r1], b[e], b_s[e], _at(pb, e))
    return m, S


def wo_linear(x, b, b_s, offs, pb=None):
    return R.wo_chain(wo_sums(x, b, b_s, offs, pb)[0])


def mm_sums(a, a_s, b, b_s, offs):
    m = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float64, device=a.device)
    S = torch.zeros_like(m)
    for e, r0, r1 in groups(offs):
        m[r0:r1], S[r0:r1] = R.mm_sums(a[r0:r1], a_s[r0:r1], b[e], b_s[e])
    return m, S


def mm_chain(m, offs, pa=None, pb=None):
    """R.mm_chain of every group's rows under that group's scales"""
    out = torch.zeros(m.shape, dtype=torch.bfloat16, device=m.device)
    for e, r0, r1 in groups(offs):
        out[r0:r1] = R.mm_chain(m[r0:r1], _at(pa, e), _at(pb, e))
    return out


def mm(a, a_s, b, b_s, offs, pa=None, pb=None):
    return mm_chain(mm_sums(a, a_s, b, b_s, offs)[0], offs, pa, pb)


def group_amax_scale(x, offs):
    """R.amax_scale per group; 0 for an empty group"""
    out = torch.zeros(offs.numel(), dtype=torch.float32, device=x.device)
    for e, r0, r1 in groups(offs):
        out[e] = R.amax_scale(x[r0:r1])
    return out


def cast(x, offs, p=None):
    """R.cast of every group's rows under p[e]; rows of no group stay zero"""
    q = torch.zeros(x.shape[0], x.shape[1] // 2, dtype=torch.uint8, device=x.device)
    s = torch.zeros(x.shape[0], x.shape[1] // 16, dtype=torch.uint8, device=x.device)
    for e, r0, r1 in groups(offs):
        q[r0:r1], s[r0:r1] = R.cast(x[r0:r1], _at(p, e))
    return q, s


def dequantize(b, b_s, pb=None, dtype=torch.bfloat16):
    """[E, N, K]"""
    return torch.stack([R.dequantize(b[e], b_s[e], _at(pb, e), dtype) for e in range(b.shape[0])])


def interval_problems(y, m64, S, K, chain):
    """(A copy of test_nvfp4_gpu.interval_problems.)  y against the float64 sum m64: every element inside [chain(m64 - d), chain(m64 + d)],
    d = 2 K 2^-24 S (the accumulation allowance of _parity.bound; the chains are monotone: their scales are positive), and the fraction
    equal to chain(m64)."""
    d = 2.0 * K * 2.0 ** -24 * S
    lo, hi, mid = (chain(v).double() for v in (m64 - d, m64 + d, m64))
    yd = y.double()
    inside = (yd >= lo) & (yd <= hi)
    eq = (yd == mid).double().mean().item() if y.numel() else 1.0
    print("%s: inside %.6f, equal %.6f" % (tuple(y.shape), inside.double().mean().item() if y.numel() else 1.0, eq))
    msgs = []
    if not bool(inside.all()):
        i, j = (int(v) for v in torch.nonzero(~inside)[0])
        msgs.append("%d elements outside the interval, first at (%d, %d): %r not in [%r, %r]"
                    % (int((~inside).sum()), i, j, yd[i, j].item(), lo[i, j].item(), hi[i, j].item()))
    return msgs, eq
