"""CPU restatement of the QAT fake quantizers (ao_amd/csrc/qat_kernels.hip): the forward in fp32, op for op, so its bf16 bytes are the
kernels' and -- tests/test_qat_host.py -- the reference's; the backward formulas in float64, which is what the kernels' fp32 sums are
held against.

    int4 (per group of g along K)   M = max, m = min, s = max(M - m, 1e-6) / 15, t = (w - m) / s, q = clamp(rint(t), 0, 15)
                                    out = bf16((q - 8) s + (m + 8 s))
    fp8  (per row)                  a = clamp(max|x|, bf16(lb), bf16(ub)), s = f32(bf16(a / 448)), t = x / s
                                    q = e4m3(clamp(t, -448, 448)), out = bf16(q s)
    backward (G = grad_out, c = 1 where the clamp passes its gradient):
    int4   ds = sum G q - sum G c t;  dm = sum G - sum G c;  dr = ds / 15 where M - m >= 1e-6 else 0
           grad = G c + [w = M] dr / #{w = M} + [w = m] (dm - dr) / #{w = m}
    fp8    ds = sum G q - sum G c t;  da = ds / 448 where lb <= max|x| <= ub else 0
           grad = G c + [|x| = max|x|] sign(x) da / #{|x| = max|x|}
"""
import math

import numpy as np
import torch

E4M3_MAX = 448.0


def bits(t):
    """bf16 tensor -> uint16 bit patterns"""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def from_bits(a):
    """uint16 bit patterns -> bf16 tensor"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).view(torch.bfloat16)


def bound(ref64, mag):
    """The gradient tolerance: |ref| 2^-8 (the final bf16 rounding, twice over) + mag 2^-16 (fp32 sums of up to 256 terms with a 256-fold
    margin); mag = sum |G| over the group or the row."""
    return ref64.abs() * 2.0 ** -8 + mag * 2.0 ** -16


# ---- int4 -------------------------------------------------------------------------------------------------------------------------------
def _int4_parts(w, g):
    n, k = w.shape
    x = w.to(torch.float32).view(n, k // g, g)
    M = torch.amax(x, dim=-1, keepdim=True)
    m = torch.amin(x, dim=-1, keepdim=True)
    s = torch.clamp(M - m, min=1e-6) / 15
    t = (x - m) / s
    r = torch.round(t)
    return x, M, m, s, t, r


def int4_fake_quantize(w, g):
    """bf16 [N, K] -> bf16 [N, K]"""
    x, M, m, s, t, r = _int4_parts(w, g)
    q = r.clamp(0, 15)
    z = m + s * 8
    return ((q - 8) * s + z).view(w.shape).to(torch.bfloat16)


def int4_codes(w, g):
    """(q in [-8, 7] fp32 [N, K/g, g], scale fp32 [N, K/g, 1], zero fp32 [N, K/g, 1]): what ao_int4_plain_quantize stores"""
    x, M, m, s, t, r = _int4_parts(w, g)
    return r.clamp(0, 15) - 8, s, m + s * 8


def int4_fake_quantize_bwd(w, grad_out, g):
    """(grad float64 [N, K], mag float64 [N, K]: sum |G| over the element's group)"""
    x, M, m, s, t, r = _int4_parts(w, g)
    G = grad_out.to(torch.float64).view(x.shape)
    c = ((r >= 0) & (r <= 15)).to(torch.float64)
    q, t64 = r.clamp(0, 15).double(), t.double()
    ds = (G * q).sum(-1, keepdim=True) - (G * c * t64).sum(-1, keepdim=True)
    dm = G.sum(-1, keepdim=True) - (G * c).sum(-1, keepdim=True)
    dr = torch.where((M - m) >= 1e-6, ds / 15, torch.zeros_like(ds))
    at_max, at_min = (x == M).double(), (x == m).double()
    grad = G * c + at_max * dr / at_max.sum(-1, keepdim=True) + at_min * (dm - dr) / at_min.sum(-1, keepdim=True)
    mag = G.abs().sum(-1, keepdim=True).expand_as(G)
    return grad.reshape(w.shape), mag.reshape(w.shape)


# ---- fp8 --------------------------------------------------------------------------------------------------------------------------------
def _bf16_bound(v, default):
    """a bound as the kernel sees it: fp32, then bf16"""
    v = default if v is None else float(v)
    return torch.tensor(v, dtype=torch.float32).to(torch.bfloat16).to(torch.float32)


def _fp8_parts(x, lb, ub):
    x32 = x.to(torch.float32).reshape(-1, x.shape[-1])
    amax = x32.abs().amax(-1, keepdim=True)
    lo, hi = _bf16_bound(lb, -math.inf), _bf16_bound(ub, math.inf)
    a = torch.minimum(torch.maximum(amax, lo), hi)
    s = (a / E4M3_MAX).to(torch.bfloat16).to(torch.float32)
    t = x32 / s
    q = t.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).to(torch.float32)
    inside = (amax >= lo) & (amax <= hi)
    return x32, amax, inside, s, t, q


def fp8_fake_quantize(x, lb=None, ub=None):
    """bf16 [..., C] -> bf16 [..., C]"""
    x32, amax, inside, s, t, q = _fp8_parts(x, lb, ub)
    return (q * s).to(torch.bfloat16).reshape(x.shape)


def fp8_codes(x, lb=None, ub=None):
    """(q fp32 [R, C] holding e4m3 values, scale fp32 [R, 1])"""
    x32, amax, inside, s, t, q = _fp8_parts(x, lb, ub)
    return q, s


def fp8_fake_quantize_bwd(x, grad_out, lb=None, ub=None):
    """(grad float64 [..., C], mag float64 [..., C]: sum |G| over the element's row)"""
    x32, amax, inside, s, t, q = _fp8_parts(x, lb, ub)
    G = grad_out.to(torch.float64).reshape(x32.shape)
    c = ((t >= -E4M3_MAX) & (t <= E4M3_MAX)).to(torch.float64)
    ds = (G * q.double()).sum(-1, keepdim=True) - (G * c * t.double()).sum(-1, keepdim=True)
    da = torch.where(inside, ds / E4M3_MAX, torch.zeros_like(ds))
    at_max = (x32.abs() == amax).double()
    grad = G * c + at_max * torch.sign(x32).double() * da / at_max.sum(-1, keepdim=True)
    mag = G.abs().sum(-1, keepdim=True).expand_as(G)
    return grad.reshape(x.shape), mag.reshape(x.shape)


def sqnr_db(got, want):
    got, want = got.double(), want.double()
    return float(10 * torch.log10(want.pow(2).sum() / (got - want).pow(2).sum()))
