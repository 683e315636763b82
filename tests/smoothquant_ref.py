"""numpy restatement of SmoothQuant as ao_amd/prototype/smoothquant and csrc/smoothquant_kernels.hip run it.  TEST INFRASTRUCTURE ONLY.  Paths
relative to the reference torchao tree; pinned against tests/golden/smoothquant.npz, which tests/golden/make_golden_smoothquant.py writes by
driving the reference's observers and its convert.

Arrays that "are bf16" are float32 arrays whose low 16 bits are zero (oracle/bf16.py); every step is ONE fp32 operation (numpy float32
arithmetic is exactly that), then a rounding to bf16 where the reference's tensor is bf16.

  col_absmax        prototype/smoothquant/core.py:53-54  max(abs(x), dim=0): exact, -0.0 counts as 0
  smoothing_factor  core.py:57-63 on bf16 [K] vectors, every tensor op rounded to bf16 in the reference's order:
                      a = bf16(x_abs_max + eps);  b = bf16(w_abs_max + eps);  p = bf16(pow(a, alpha));  q = bf16(pow(b, 1 - alpha));  s = bf16(p / q)
                    pow is the one step that is not correctly rounded everywhere: fp32 pow here (through float64, rounded to fp32), and an
                    fp32 pow that differs in its last places can move the bf16 rounding by at most one step
  pre_scale         api.py:159  bf16(1 / s)
  smoothed_amax     core.py:66-68, 192-195  max |bf16(f32(x) / f32(s))|
  prescaled         int8_tensor.py:278  t = bf16(f32(x) * f32(pre)): the product of two bf16 values is exact in fp32, one rounding
  quantize_*        oracle/int8_ref.py (the int8 chains of the existing casts) on t
  static / running activation scale: see static_scale, running_scale
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import bf16, int8_ref as I8  # noqa: E402

F32 = np.float32
EPS = F32(np.finfo(np.float32).eps)


def col_absmax(x, state=None):
    """fp32 [K]: max(state, max_m |x[m, k]|); state defaults to zeros"""
    x = np.asarray(x, F32).reshape(-1, np.shape(x)[-1])
    m = np.abs(x).max(axis=0) if x.shape[0] else np.zeros(x.shape[1], F32)
    m = m + F32(0)  # (-0.0 -> +0.0; abs has already cleared the sign)
    return m.astype(F32) if state is None else np.maximum(np.asarray(state, F32), m).astype(F32)


def _pow32(a, e):
    with np.errstate(all="ignore"):
        return np.power(np.asarray(a, np.float64), np.float64(F32(e))).astype(F32)


def smoothing_factor(x_abs_max, w_abs_max, alpha):
    """bf16 [K] (as fp32).  alpha None: ones."""
    x_abs_max, w_abs_max = np.asarray(x_abs_max, F32), np.asarray(w_abs_max, F32)
    assert bf16.is_bf16(x_abs_max) and bf16.is_bf16(w_abs_max)
    if alpha is None:
        return np.ones_like(x_abs_max)
    a, b = bf16.add(x_abs_max, EPS), bf16.add(w_abs_max, EPS)
    p, q = bf16.bf16_round(_pow32(a, alpha)), bf16.bf16_round(_pow32(b, 1 - alpha))
    return bf16.div(p, q)


def pre_scale(s):
    """act_pre_scale = bf16(1 / s)"""
    return bf16.div(F32(1.0), np.asarray(s, F32))


def smoothed_weight(W, s):
    """bf16(W * s): the weight the base handler quantizes (api.py:131)"""
    return bf16.mul(np.asarray(W, F32), np.asarray(s, F32)[None, :])


def smoothed_amax(x, s, state=0.0):
    """fp32 scalar: max(state, max |bf16(x / s)|)"""
    x = np.asarray(x, F32).reshape(-1, np.shape(x)[-1])
    if x.shape[0] == 0:
        return F32(state)
    t = bf16.div(x, np.asarray(s, F32)[None, :])
    return F32(max(F32(state), np.abs(t).max()))


def prescaled(x, pre):
    """t = bf16(x * pre), bf16 [M, K] as fp32"""
    x, pre = np.asarray(x, F32), np.asarray(pre, F32)
    assert bf16.is_bf16(x) and bf16.is_bf16(pre)
    with np.errstate(all="ignore"):
        return bf16.bf16_round((x * pre[None, :]).astype(F32))


def quantize_rowwise_prescaled(x, pre):
    """(q int8 [M, K], scale fp32 [M])"""
    return I8.quantize_rowwise(prescaled(x, pre))


def quantize_tensorwise_prescaled(x, pre):
    """(q int8 [M, K], scale fp32 scalar)"""
    return I8.quantize_tensorwise(prescaled(x, pre))


def quantize_static(t, scale, zp=None):
    """clip(rint(t * f32(1 / scale)) + zp, -128, 127); scale / zp of 1 or M entries (Int8Tensor.from_hp with given qparams,
    int8_tensor.py:212-231)"""
    inv = (F32(1.0) / np.asarray(scale, F32)).astype(F32).reshape(-1, 1)
    z = np.zeros((1, 1), F32) if zp is None else np.asarray(zp, F32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        q = np.rint((np.asarray(t, F32) * inv).astype(F32)).astype(F32) + z
    return np.clip(q, -128, 127).astype(np.int8)


def quantize_static_prescaled(x, pre, scale, zp=None):
    return quantize_static(prescaled(x, pre), scale, zp)


def static_scale(amax):
    """The default observer's activation scale: Int8Tensor.from_hp(x / s, PerTensor())'s, max(bf16(amax / 127.5), eps) (fp32 scalar)"""
    return F32(max(bf16.div(F32(amax), F32(127.5)).reshape(()), EPS))


def running_scale(amax):
    """The running observer's activation scale (core.py:295-300): abs_max / 127.5 clamped at fp32 eps, in the dtype of the smoothed
    activation -- bf16 here, so the quotient is rounded to bf16 like every bf16 tensor op."""
    return F32(max(bf16.div(F32(amax), F32(127.5)).reshape(()), EPS))


def quantize_weight(Ws, per_tensor=False):
    """Int8Tensor.from_hp(Ws, PerRow() | PerTensor()): (qdata int8 [N, K], scale fp32 [N] or scalar)"""
    return I8.quantize_tensorwise(Ws) if per_tensor else I8.quantize_rowwise(Ws)
