"""The W4A8 contract (ao_amd/csrc/da8w4_kernels.hip states it) restated in numpy (TEST INFRASTRUCTURE ONLY): the casts (qparams in bf16
tensor arithmetic, codes in fp32), a float64 linear on given codes, the device layouts, the case list.  make_golden_da8w4.py asserts that the
casts give torchao's bytes.  bf16 arrays are uint16 bit patterns at the interfaces, bf16-valued float32 inside (oracle/bf16.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import bf16  # noqa: E402

F32 = np.float32
GROUPS = (32, 64, 128)
WEIGHT_EPS, ACT_EPS = bf16.bf16_round(F32(1e-6)), F32(2.0 ** -23)  # clamp(bf16 tensor, min=1e-6) compares in bf16; finfo(float32).eps

LINEAR_M, LINEAR_N = (1, 16, 17, 65, 129), (32, 96)  # the tiled form's tile is 128 rows x 64 columns, a K step is 128


LINEAR_K = {g: (g, 2 * g, 128 + g, 384 + g) for g in GROUPS}  # g, 2 g, one K step + g, three K steps + g


def _asym(mn, mx, qmax, eps):
    s = np.maximum(bf16.div(bf16.sub(mx, mn), F32(qmax)), eps)
    zp = np.clip(bf16.sub(F32(0), np.rint(bf16.div(mn, s))), 0, qmax)
    return s.astype(F32), zp.astype(np.int32)


def _codes(v, s, zp, lo, hi):
    return np.clip(np.rint(v * (F32(1) / s)) + zp.astype(F32), lo, hi)


def weight_cast(w_bits, g):
    """from_hp_da8w4's cast of bf16 w [N, K] -> (codes uint8 [N, K] in 0 .. 15, scale float32 [N, G], zero_point int32 [N, G])"""
    n, k = w_bits.shape
    w = bf16.from_bits(np.asarray(w_bits)).reshape(n, k // g, g)
    s, zp = _asym(np.minimum(w.min(axis=2), F32(0)), np.maximum(w.max(axis=2), F32(0)), 15, WEIGHT_EPS)
    return _codes(w, s[..., None], zp[..., None], 0, 15).astype(np.uint8).reshape(n, k), s, zp


def act_cast(x_bits, symmetric):
    """_da8w4_linear's per-token cast of bf16 x [M, K] -> (codes uint8 0 .. 255, or int8 +-127 when symmetric; scale f32 [M]; zero_point [M])"""
    x = bf16.from_bits(np.asarray(x_bits))
    mn, mx = np.minimum(x.min(axis=1), F32(0)), np.maximum(x.max(axis=1), F32(0))
    if symmetric:
        s = np.maximum(bf16.div(np.maximum(-mn, mx), F32(127)), ACT_EPS).astype(F32)
        zp = np.zeros(x.shape[0], np.int32)
        return _codes(x, s[:, None], zp[:, None], -127, 127).astype(np.int8), s, zp
    s, zp = _asym(mn, mx, 255, ACT_EPS)
    return _codes(x, s[:, None], zp[:, None], 0, 255).astype(np.uint8), s, zp


def group_sums(qa, za, qw, zw):
    """I_g [G, M, N] int64: the exact sums of the contract"""
    m, k = qa.shape
    n, gcount = zw.shape
    a = (qa.astype(np.int64) - za.astype(np.int64)[:, None]).reshape(m, gcount, -1)
    w = (qw.astype(np.int64).reshape(n, gcount, -1) - zw.astype(np.int64)[..., None])
    return np.einsum("mgk,ngk->gmn", a, w)


def linear64(qa, sa, za, qw, sw, zw, bias_bits=None):
    """float64 (y, mag) [M, N]: y = sa * sum_g I_g sw + bias, mag = sa * sum_g |I_g| sw + |bias|"""
    ig = group_sums(qa, za, qw, zw).astype(np.float64)
    s = sw.astype(np.float64).T[:, None, :]
    y = (ig * s).sum(axis=0) * sa.astype(np.float64)[:, None]
    mag = (np.abs(ig) * s).sum(axis=0) * sa.astype(np.float64)[:, None]
    if bias_bits is not None:
        b = bf16.from_bits(np.asarray(bias_bits)).astype(np.float64)[None, :]
        y, mag = y + b, mag + np.abs(b)
    return y, mag


def bound(ref, mag, groups):
    """one bf16 rounding of the result, G + 3 fp32 roundings on terms bounded by mag, a factor 2 of slack"""
    return 2.0 ** -8 * np.abs(ref) + (groups + 4) * 2.0 ** -23 * mag


# ---- the device layouts ----
def pack_weight(qw):
    """codes [N, K] -> int32 [N, Kp / 8]: byte 16 kq + 4 d + j of a 128-k superblock holds k = 64 t + 32 (d >> 1) + 8 kq + 4 (d & 1) + j in nibble t"""
    n, k = qw.shape
    kp = (k + 127) // 128 * 128
    q = np.zeros((n, kp), np.uint8)
    q[:, :k] = qw
    q = q.reshape(n, kp // 128, 2, 2, 4, 2, 4)  # sb, t, h, kq, d & 1, j
    by = q[:, :, 0] | (q[:, :, 1] << 4)         # sb, h, kq, dl, j
    return np.ascontiguousarray(by.transpose(0, 1, 3, 2, 4, 5)).reshape(n, kp // 2).view(np.int32)


def weight_meta(qw, sw, zw):
    """(scale_and_zero float32 [G, N, 2], qzeros int8 [G, N], compensation int16 [G, N])"""
    n, gcount = zw.shape
    comp = (qw.astype(np.int32).reshape(n, gcount, -1) - zw[..., None]).sum(axis=2)
    word = ((comp.astype(np.uint32) << 16) | zw.astype(np.uint32)).astype(np.uint32)
    sz = np.stack([sw.astype(F32).view(np.uint32), word], axis=2).transpose(1, 0, 2)
    return np.ascontiguousarray(sz).view(F32), np.ascontiguousarray(zw.T).astype(np.int8), np.ascontiguousarray(comp.T).astype(np.int16)


def act_device(qa, za, g, symmetric):
    """(codes int8 [M, Kp], act_meta int32 [M, Gp]) as the activation cast leaves them"""
    m, k = qa.shape
    shift = 0 if symmetric else 128
    a = qa.astype(np.int32) - shift
    kp, gp = (k + 127) // 128 * 128, (k // g + 3) // 4 * 4
    codes = np.zeros((m, kp), np.int8)
    codes[:, :k] = a
    meta = np.zeros((m, gp), np.uint32)
    sums = a.reshape(m, k // g, g).sum(axis=2)
    meta[:, :k // g] = ((-sums).astype(np.uint32) & 0xFFFF) | ((-(za.astype(np.int32) - shift)).astype(np.uint32)[:, None] << 16)
    return codes, meta.view(np.int32)
