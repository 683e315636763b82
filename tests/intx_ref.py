"""The Intx contracts (ao_amd/csrc/intx_kernels.hip states them) restated in numpy: the reference's bf16 tensor arithmetic, every step ONE
fp32 operation rounded once to bf16, nearest even (TEST INFRASTRUCTURE ONLY).  tests/golden/make_golden_intx.py asserts that this file gives
the bytes of torchao's IntxUnpackedToInt8Tensor.from_hp / dequantize and _apply_int8_act_asym_per_token_quant_dequant on the CPU.

bf16 arrays are uint16 bit patterns at the interfaces and bf16-valued float32 inside (oracle/bf16.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import bf16  # noqa: E402

MAPPINGS = ("SYMMETRIC", "SYMMETRIC_NO_CLIPPING_ERR", "ASYMMETRIC")
EPS = np.float32(2.0 ** -126)  # torch.finfo(torch.bfloat16).smallest_normal
NAN_BITS = 0x7FC0              # every NaN is stored as this one (the recording canonicalises the reference's, whose payload depends on
                               # whether a vector or a scalar loop converted it)


def bounds(b):
    return -(1 << (b - 1)), (1 << (b - 1)) - 1


def _clamp_min(s):
    return np.where(np.isnan(s), s, np.maximum(s, EPS))  # torch.clamp keeps NaN


def qparams(w_bits, b, mapping, g):
    """choose_qparams_affine on bf16 w [N, K] in groups of g along K -> (scale bits uint16 [N, K/g], zero_point int8 [N, K/g])"""
    qmin, qmax = bounds(b)
    w = bf16.from_bits(np.asarray(w_bits)).reshape(w_bits.shape[0], -1, g)
    mn = np.minimum(w.min(axis=2), np.float32(0))
    mx = np.maximum(w.max(axis=2), np.float32(0))
    with np.errstate(all="ignore"):
        if mapping == "ASYMMETRIC":
            s = _clamp_min(bf16.div(bf16.sub(mx, mn), np.float32(qmax - qmin)))
            zp = np.clip(bf16.sub(np.float32(qmin), np.rint(bf16.div(mn, s))), qmin, qmax)
        else:
            if mapping == "SYMMETRIC":
                s = bf16.div(np.maximum(-mn, mx), np.float32((qmax - qmin) / 2))
            else:
                smin, smax = bf16.div(mn, np.float32(qmin)), bf16.div(mx, np.float32(qmax))
                s = np.where(smin > smax, smin, smax)
            s = _clamp_min(s)
            zp = np.zeros_like(s)
    sb = np.where(np.isnan(s), np.uint16(NAN_BITS), bf16.to_bits(np.where(np.isnan(s), np.float32(0), s))).astype(np.uint16)
    return sb, zp.astype(np.int8)


def quantize(w_bits, scale_bits, zp, b):
    """quantize_affine: clamp(rint(bf16(w * bf16(1 / s))) + zp, qmin, qmax) in bf16 -> int8 [N, K]; a NaN (a NaN scale) stores 0"""
    qmin, qmax = bounds(b)
    n, k = w_bits.shape
    g = k // scale_bits.shape[1]
    w = bf16.from_bits(np.asarray(w_bits)).reshape(n, -1, g)
    with np.errstate(all="ignore"):
        inv = bf16.div(np.float32(1), bf16.from_bits(scale_bits))[..., None]
        q = bf16.add(np.rint(bf16.mul(w, inv)), zp.astype(np.float32)[..., None])
        q = np.where(np.isnan(q), np.float32(0), np.clip(q, qmin, qmax))
    return q.astype(np.int8).reshape(n, k)


def dequantize(q, scale_bits, zp):
    """dequantize_affine: bf16((q - zp) * s) -> bf16 bits [N, K]"""
    n, k = q.shape
    g = k // scale_bits.shape[1]
    d = (q.astype(np.float32).reshape(n, -1, g) - zp.astype(np.float32)[..., None])
    with np.errstate(all="ignore"):
        out = bf16.mul(d, bf16.from_bits(scale_bits)[..., None]).reshape(n, k)
    nan = np.isnan(out)
    return np.where(nan, np.uint16(NAN_BITS), bf16.to_bits(np.where(nan, np.float32(0), out))).astype(np.uint16)


def from_hp(w_bits, b, mapping, g):
    s, zp = qparams(w_bits, b, mapping, g)
    return quantize(w_bits, s, zp, b), s, zp


def act_fake_quant(x_bits):
    """_apply_int8_act_asym_per_token_quant_dequant on bf16 x [M, K] -> bf16 bits [M, K]"""
    k = x_bits.shape[1]
    q, s, zp = from_hp(x_bits, 8, "ASYMMETRIC", k)
    return dequantize(q, s, zp)


def pack_fields(b):
    """the bit fields of a b-bit code, low bits first: (width, shift) pairs"""
    return {1: [(1, 0)], 2: [(2, 0)], 3: [(2, 0), (1, 2)], 4: [(4, 0)], 5: [(4, 0), (1, 4)], 6: [(4, 0), (2, 4)], 7: [(4, 0), (2, 4), (1, 6)],
            8: [(8, 0)]}[b]


def pack(q, b):
    """The device layout: per row and run of 32 weights, b dwords = one plane per field; inside a plane of width f
    the dword d holds weights 8 * (4 / f) * d ... and byte j of it, bit position f * t, holds weight 32 / f * d + 4 t + j."""
    n, k = q.shape
    u = (q.astype(np.int32) - bounds(b)[0]).astype(np.uint32).reshape(n, k // 32, 32)
    if b == 8:  # the plain byte array, signed: what the unpacked tensor's qdata is
        return np.ascontiguousarray(q).view(np.int32)
    planes = []
    for f, sh in pack_fields(b):
        v = (u >> sh) & ((1 << f) - 1)
        per = 32 // f  # weights a dword
        dw = np.zeros((n, k // 32, f), dtype=np.uint32)
        for d in range(f):
            for t in range(8 // f):
                for j in range(4):
                    dw[:, :, d] |= v[:, :, per * d + 4 * t + j] << (8 * j + f * t)
        planes.append(dw)
    return np.concatenate(planes, axis=2).reshape(n, (k // 32) * b).view(np.int32)
