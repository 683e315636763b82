"""numpy restatement of torchao's blockwise float8 linear: 1 x 128 activation blocks, 128 x 128 weight blocks, fp32 scales.
TEST INFRASTRUCTURE ONLY.  Paths relative to the reference torchao tree.  The casts and dequantize are pinned against
tests/golden/fp8_block.npz, which tests/golden/make_golden_fp8_block.py writes from the reference on the CPU; the reference's GEMM is a
Triton kernel that does not run there, so the GEMM's yardsticks are the float64 sum and the fp32 chain below.

  cast   quantization/quantize_/workflows/float8/float8_tensor.py:233-242 -> quant_primitives.py:2173-2212 (_choose_scale_float8),
         :2271-2287 (_quantize_affine_float8):  scale = f32(bf16(amax_block / 448)), q = e4m3_sat(f32(x) / scale); a block of zeros
         gives scale 0 and NaN codes
  deq    float8_tensor.py:255-275: (f32(q) * scale expanded block by block).to(bf16)
  GEMM   quantize_/workflows/float8/kernels.py:85-97, float8_tensor.py:433-447, per output element in fp32:
         acc = 0;  for kb ascending: acc += (p_kb * a_s[m][kb]) * b_s[n // 128][kb], p_kb the sum of the block's 128 products;
         t = bf16(acc);  y = bias ? bf16(f32(t) + f32(bias[n])) : t

bf16 tensors are uint16 bit patterns, e4m3 codes uint8, scales float32.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import bf16, fp8_ref  # noqa: E402

BLOCK = 128


def _cast(xb, br, bc):
    x = bf16.from_bits(np.asarray(xb, dtype=np.uint16))
    R, C = x.shape
    assert R % br == 0 and C % bc == 0, f"shape {x.shape} is not divisible by the block {(br, bc)}"
    amax = np.abs(x).reshape(R // br, br, C // bc, bc).max(axis=(1, 3))
    scale = bf16.div(amax.astype(np.float32), fp8_ref.E4M3_MAX).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (x / expand(scale, br, bc)).astype(np.float32)
    t = np.clip(t, -fp8_ref.E4M3_MAX, fp8_ref.E4M3_MAX)  # NaN stays NaN
    return fp8_ref.f32_to_e4m3(t), scale


def expand(scale, br, bc):
    """Block scales [R/br][C/bc] -> one per element [R][C] (_maybe_expand_scale_to_tensor_shape)."""
    return np.repeat(np.repeat(np.asarray(scale, dtype=np.float32), br, axis=0), bc, axis=1)


def cast_1x128(xb):
    """x bf16 bits [M, K] -> (codes uint8 [M, K], scale fp32 [M, K/128])."""
    return _cast(xb, 1, BLOCK)


def cast_128x128(wb):
    """w bf16 bits [N, K] -> (codes uint8 [N, K], scale fp32 [N/128, K/128])."""
    return _cast(wb, BLOCK, BLOCK)


def dequantize(q, scale, br, bc):
    """bf16 bits of f32(q) * scale, the scale expanded block by block."""
    with np.errstate(invalid="ignore"):
        v = fp8_ref.e4m3_to_f32(q) * expand(scale, br, bc)
    return bf16.to_bits(bf16.bf16_round(v.astype(np.float32)))


def is_nan_code(q):
    return (np.asarray(q, dtype=np.uint8) & 0x7F) == 0x7F


def same_codes(q, ref):
    """NaN codes compare as NaN whatever the sign bit (the reference's 0 / 0 is 0xFF, a cast of +NaN 0x7F)."""
    q, ref = np.asarray(q, dtype=np.uint8), np.asarray(ref, dtype=np.uint8)
    return bool(np.array_equal(is_nan_code(q), is_nan_code(ref)) and np.array_equal(np.where(is_nan_code(q), 0, q), np.where(is_nan_code(ref), 0, ref)))


def _block_products(aq, bq):
    """p[kb][m][n]: the float64 sum of each K block's 128 products."""
    a = fp8_ref.e4m3_to_f32(aq).astype(np.float64)
    b = fp8_ref.e4m3_to_f32(bq).astype(np.float64)
    kb = a.shape[1] // BLOCK
    return [a[:, i * BLOCK:(i + 1) * BLOCK] @ b[:, i * BLOCK:(i + 1) * BLOCK].T for i in range(kb)], a, b


def _b_rows(b_s, N):
    """b_s [ceil(N/128)][K/128] -> one row of scales per output column [N][K/128]."""
    b_s = np.asarray(b_s, dtype=np.float32)
    assert b_s.shape[0] == (N + BLOCK - 1) // BLOCK
    return np.repeat(b_s, BLOCK, axis=0)[:N]


def linear_f64(aq, a_s, bq, b_s):
    """(y, S) in float64 with the scales applied: y = sum_kb p_kb a_s[m][kb] b_s[n // 128][kb]; S the same sum of absolute products."""
    p, a, b = _block_products(aq, bq)
    a_s = np.asarray(a_s, dtype=np.float64)
    bs = _b_rows(b_s, bq.shape[0]).astype(np.float64)
    y = np.zeros((aq.shape[0], bq.shape[0]), dtype=np.float64)
    S = np.zeros_like(y)
    for i, pi in enumerate(p):
        w = a_s[:, i][:, None] * bs[:, i][None, :]
        y += pi * w
        S += (np.abs(a[:, i * BLOCK:(i + 1) * BLOCK]) @ np.abs(b[:, i * BLOCK:(i + 1) * BLOCK]).T) * np.abs(w)
    return y, S


def chain_bits(aq, a_s, bq, b_s, bias_bits=None):
    """The fp32 chain, bf16 bits [M, N].  p_kb is the float64 block sum rounded to fp32 (exact whenever the block's partial sums are
    exact in fp32, as in the exact-sum tests)."""
    p, _, _ = _block_products(aq, bq)
    a_s = np.asarray(a_s, dtype=np.float32)
    bs = _b_rows(b_s, bq.shape[0])
    acc = np.zeros((aq.shape[0], bq.shape[0]), dtype=np.float32)
    for i, pi in enumerate(p):
        t = (pi.astype(np.float32) * a_s[:, i][:, None]).astype(np.float32)
        u = (t * bs[:, i][None, :]).astype(np.float32)
        acc = (acc + u).astype(np.float32)
    return add_bias_bits(bf16.to_bits(bf16.bf16_round(acc)), bias_bits)


def add_bias_bits(y_bits, bias_bits):
    """bf16(f32(y) + f32(bias[n])) on bf16 bits; y itself without a bias."""
    if bias_bits is None:
        return np.asarray(y_bits, dtype=np.uint16)
    return bf16.to_bits(bf16.add(bf16.from_bits(y_bits), bf16.from_bits(bias_bits)[None, :]))
