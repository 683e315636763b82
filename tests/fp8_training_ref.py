"""numpy restatement of torchao.float8's dynamic training cast (hp_tensor_to_float8_dynamic).  TEST INFRASTRUCTURE ONLY.  Paths relative
to the reference torchao tree.  Pinned byte for byte against tests/golden/fp8_training.npz, which tests/golden/make_golden_fp8_training.py
writes from the reference on the CPU.

  amax   float8/float8_utils.py:56-82:  max |x| over the tensor (axis None), or along one axis with keepdim
  scale  float8/float8_utils.py:31-53:  f32(448 / max(f64(amax), 1e-12)) -- the division in float64, ONE rounding to fp32;
         :244-246 with round_scales_to_power_of_2: exp2(floor(log2(scale))), here the mantissa bits cleared (every scale the formula
         gives from a bf16 amax is a normal fp32; the fixture's recorder asserts the two agree on everything it records)
  cast   float8/float8_training_tensor.py:153-154, float8/float8_utils.py:118-139:  e4m3fn_rne(clamp(f32(x) * scale, -448, 448))
  1/s    float8/float8_ops.py:44-45:  fp32 1 / scale, what the GEMM multiplies by

bf16 tensors are uint16 bit patterns, e4m3 codes uint8, scales float32.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import bf16, fp8_ref  # noqa: E402

EPS = 1e-12


def clear_mantissa(scale):
    """exp2(floor(log2(scale))) of a normal fp32."""
    return (np.asarray(scale, dtype=np.float32).view(np.uint32) & np.uint32(0xFF800000)).view(np.float32)


def amax_to_scale(amax, pow2=False):
    s = (448.0 / np.maximum(np.asarray(amax, dtype=np.float32).astype(np.float64), EPS)).astype(np.float32)
    return clear_mantissa(s) if pow2 else s


def cast(xb, axis=None, pow2=False):
    """x (bf16 bits [R, C]) cast with one scale per slice along `axis` (-1 / 1: per row, scale [R, 1]; 0: per column, scale [1, C]; None:
    one for the tensor, scale []) -> (codes uint8 [R, C], scale fp32, inv_scale fp32)."""
    x = bf16.from_bits(np.asarray(xb, dtype=np.uint16)).astype(np.float32)
    return cast_under(xb, np.abs(x).max() if axis is None else np.abs(x).max(axis=axis, keepdims=True), pow2)


def cast_under(xb, amax, pow2=False):
    """The same cast under a GIVEN amax (fp32, broadcast against x: [R, 1], [1, C] or []), which need not be x's own."""
    x = bf16.from_bits(np.asarray(xb, dtype=np.uint16)).astype(np.float32)
    scale = amax_to_scale(amax, pow2)
    with np.errstate(over="ignore"):  # (under an amax below x's own a product may overflow: inf, clamped to 448 like any other)
        t = np.clip((x * scale).astype(np.float32), -fp8_ref.E4M3_MAX, fp8_ref.E4M3_MAX)
    return fp8_ref.f32_to_e4m3(t), scale, (np.float32(1.0) / scale).astype(np.float32)


def dequant(q, scale):
    """The value a code stands for, as float64: f32(code) / scale."""
    return fp8_ref.e4m3_to_f32(q).astype(np.float64) / np.asarray(scale, dtype=np.float64)
