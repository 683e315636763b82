"""numpy restatement of the MXFP4 cast, MX dequantisation and the MX dense linear.
TEST INFRASTRUCTURE ONLY.  Paths relative to the reference torchao tree.  Pinned against tests/golden/mx_linear.npz, which
tests/golden/make_golden_mx_linear.py writes from the reference.

  to_mx(x, float4_e2m1fn_x2, 32, mode)      prototype/mx_formats/mx_tensor.py:228-409 (RCEIL :161-224)
  e2m1 rounding                             prototype/custom_fp_utils.py:27-140 (_f32_to_floatx_unpacked(x, 2, 1))
  packing                                   prototype/mx_formats/kernels.py:155-160 (pack_uint4)
  MXTensor.dequantize                       mx_tensor.py:412-471, :600-628
  linear                                    out = sum_k dq(a) dq(b) + bias, in float64 here
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import bf16  # noqa: E402
from oracle.fp8_ref import e4m3_to_f32  # noqa: E402
from oracle.mx_ref import BLOCK, FLOOR, RCEIL, e8m0_reciprocal_f32, f32_to_e8m0_rceil  # noqa: E402
from oracle.mx_ref import to_mx as to_mx8  # noqa: E402,F401

E2M1_VALUES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], dtype=np.float32)
FMT_E4M3, FMT_E2M1 = 0, 4


def f32_to_e2m1(bits):
    """_f32_to_floatx_unpacked(x, ebits=2, mbits=1) on fp32 bit patterns (uint32) -> codes uint8 (sign in bit 3)."""
    bits = np.asarray(bits, dtype=np.uint32)
    sign = ((bits >> 28) & 8).astype(np.uint8)
    a = bits & np.uint32(0x7FFFFFFF)
    x = a.view(np.float32)
    with np.errstate(invalid="ignore"):
        sat = x >= np.float32(6.0)
        den = ~sat & (x < np.float32(1.0))
    den_code = ((x + np.float32(2.0 ** 22)).astype(np.float32).view(np.uint32) - np.uint32(149 << 23)) & np.uint32(0xFF)
    norm_code = ((a + np.uint32(0xC1000000 + 0x1FFFFF) + ((a >> 22) & np.uint32(1))) >> np.uint32(22)) & np.uint32(0xFF)
    code = np.where(sat, 7, np.where(den, den_code, norm_code)).astype(np.uint8)
    return code | sign


def fp4_block_exponent(amax, mode):
    amax = np.asarray(amax, dtype=np.float32)
    if mode == RCEIL:
        return f32_to_e8m0_rceil((amax * np.float32(1.0 / 6.0)).astype(np.float32))
    ex = ((amax.view(np.uint32) >> 23) & 0xFF).astype(np.int32) - 127 - 2
    e = (np.clip(ex, -127, 128) + 127).astype(np.uint8)
    return np.where(np.isfinite(amax), e, 255).astype(np.uint8)


def to_mx4(x_bits, mode=RCEIL):
    """to_mx(x, float4_e2m1fn_x2, 32, mode) for bf16 x given as uint16 bit patterns [..., K].
    Returns (packed codes uint8 [..., K/2], scale e8m0 uint8 [..., K/32])."""
    x_bits = np.asarray(x_bits, dtype=np.uint16)
    shp = x_bits.shape
    xb = (x_bits.reshape(-1, BLOCK).astype(np.uint32) << 16)
    xf = xb.view(np.float32)
    with np.errstate(invalid="ignore"):
        amax = np.abs(xf).max(axis=1).astype(np.float32)  # NaN propagates like torch.amax
    e = fp4_block_exponent(amax, mode)
    r = e8m0_reciprocal_f32(e)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        prod = (xf * r[:, None]).astype(np.float32).view(np.uint32)
    # non-finite blocks: the reciprocal is the NaN 0x7F800001 and every product is that NaN, quieted (0x7FC00001), whatever the element
    # -- NaN elements included (the reference's CPU bytes: code 3 throughout)
    prod = np.where((e == 255)[:, None], np.uint32(0x7FC00001), prod)
    codes = f32_to_e2m1(prod).reshape(shp)
    packed = (codes[..., 0::2] | (codes[..., 1::2] << 4)).astype(np.uint8)
    return packed, e.reshape(*shp[:-1], shp[-1] // BLOCK)


def unpack_e2m1(packed):
    packed = np.asarray(packed, dtype=np.uint8)
    out = np.empty((*packed.shape[:-1], packed.shape[-1] * 2), dtype=np.uint8)
    out[..., 0::2] = packed & 0xF
    out[..., 1::2] = packed >> 4
    return out


def element_values(codes, fmt):
    """codes -> fp32 element values ([..., K] from e4m3 [..., K] or packed e2m1 [..., K/2])."""
    if fmt == FMT_E2M1:
        return E2M1_VALUES[unpack_e2m1(codes)]
    return e4m3_to_f32(np.asarray(codes, dtype=np.uint8))


def scale_values(scale):
    s = np.exp2(scale.astype(np.float64) - 127.0)
    return np.where(scale == 255, np.nan, s)


def dequantize_bf16(codes, scale, fmt):
    """MXTensor.dequantize(bf16): bf16(element) * bf16(2^(e - 127)), NaN where the scale byte is 255 -> bf16 bit patterns."""
    v = element_values(codes, fmt)
    s = scale_values(scale).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return bf16.to_bits(bf16.mul(v, np.repeat(s, BLOCK, axis=-1)))


def dequantize_f64(codes, scale, fmt):
    v = element_values(codes, fmt).astype(np.float64)
    return v * np.repeat(scale_values(scale), BLOCK, axis=-1)


def linear_f64(a_codes, a_scale, b_codes, b_scale, fmt, bias_bits=None):
    """sum_k dq(a)[m, k] dq(b)[n, k] (+ bias[n]) in float64, and sum_k |dq(a) dq(b)| (the size of the terms, for parity bounds)."""
    a = dequantize_f64(a_codes, a_scale, fmt)
    b = dequantize_f64(b_codes, b_scale, fmt)
    with np.errstate(invalid="ignore", over="ignore"):
        y = a @ b.T
        mag = np.abs(a) @ np.abs(b).T
    if bias_bits is not None:
        bb = bf16.from_bits(bias_bits).astype(np.float64)
        y = y + bb[None, :]
        mag = mag + np.abs(bb)[None, :]
    return y, mag


def quantize(x_bits, fmt, mode=RCEIL):
    """(codes, scales) of the 1 x 32 cast for fmt, x given as bf16 bit patterns."""
    if fmt == FMT_E2M1:
        return to_mx4(x_bits, mode)
    return to_mx8(bf16.from_bits(x_bits), mode)


def emulated_linear_bf16(a_codes, a_scale, b_codes, b_scale, fmt, bias_bits=None):
    """KernelPreference.EMULATED (mx_tensor.py:828-841): both operands dequantised to bf16, then aten mm / addmm, one bf16 rounding of
    the exact sum (pinned against the reference's CPU output in the fixture) -> bf16 bit patterns."""
    a = bf16.from_bits(dequantize_bf16(a_codes, a_scale, fmt)).astype(np.float64)
    b = bf16.from_bits(dequantize_bf16(b_codes, b_scale, fmt)).astype(np.float64)
    y = a @ b.T
    if bias_bits is not None:
        y = y + bf16.from_bits(bias_bits).astype(np.float64)[None, :]
    return bf16.to_bits(bf16.bf16_round(y.astype(np.float32)))
