"""numpy restatement of torchao's blockwise float8 TRAINING casts and of its weight-gradient GEMM.  TEST INFRASTRUCTURE ONLY.  Paths
relative to the reference torchao tree.  The casts are pinned byte for byte against tests/golden/blockwise_fp8_training.npz, which
tests/golden/make_golden_blockwise_fp8_training.py writes from the reference's torch functions on the CPU; the reference's GEMMs are
Triton kernels or cuBLAS calls that do not run there, so the GEMM's yardsticks are the float64 sum and the fp32 chain below.

  casts  prototype/blockwise_fp8_training/kernels.py
           :1031-1058 torch_blockwise_scale_act_quant_lhs   1 x 128 blocks   -> cast_rows
           :1061-1118 torch_blockwise_scale_act_quant_rhs   128 x 1 blocks   -> cast_cols (stored transposed, as the HIP cast writes it)
           :1121-1156 torch_blockwise_scale_weight_quant    128 x 128 blocks -> cast_weight
         scale = f32(448 / max(f64(amax), 1e-12)): the division in float64, ONE rounding to fp32;  q = e4m3fn_rne(clamp(f32(x) * scale,
         -448, 448));  the functions return 1 / scale in fp32.  A block of zeros: scale f32(448 / 1e-12), codes 0, no NaN.
         The 128 x 1 function clamps the amax at 1e-12 while it is still bf16 (:1096, torch.clamp before .to(float64)): there the floor is
         bf16(1e-12) = 0x2B8D = 1.00186e-12, and only the reciprocal of a block below it shows the difference.
  GEMM   kernels.py:320-379 (triton_fp8_gemm_1x128_128x1), per output element in fp32:
         acc = 0;  for mb ascending: acc += (p_mb * g_inv[mb][n]) * x_inv[mb][k], p_mb the sum of the token block's 128 products;
         out = bf16(acc)

bf16 tensors are uint16 bit patterns, e4m3 codes uint8, scales float32.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import bf16, fp8_ref  # noqa: E402

BLOCK = 128
EPS = 1e-12
EPS_BF16 = np.array([0x2B8D0000], dtype=np.uint32).view(np.float32)[0]  # 1e-12 rounded to bf16


def _f32(xb):
    return bf16.from_bits(np.asarray(xb, dtype=np.uint16)).astype(np.float32)


def scale_of(amax, clamp_in_bf16=False):
    a = np.asarray(amax, dtype=np.float32)
    if clamp_in_bf16:
        a = np.maximum(a, EPS_BF16)
    return (448.0 / np.maximum(a.astype(np.float64), EPS)).astype(np.float32)


def _codes(x, scale):
    t = np.clip((x * scale).astype(np.float32), -fp8_ref.E4M3_MAX, fp8_ref.E4M3_MAX)
    return fp8_ref.f32_to_e4m3(t)


def _inv(scale):
    return (np.float32(1.0) / scale).astype(np.float32)


def cast_rows(xb):
    """x bf16 bits [R, C] -> (codes uint8 [R, C], inv fp32 [R, C/128], scale fp32 [R, C/128]): 1 x 128 blocks."""
    x = _f32(xb)
    R, C = x.shape
    assert C % BLOCK == 0
    s = scale_of(np.abs(x).reshape(R, C // BLOCK, BLOCK).max(axis=2))
    return _codes(x, np.repeat(s, BLOCK, axis=1)), _inv(s), s


def cast_cols(xb):
    """x bf16 bits [R, C] -> (codes uint8 TRANSPOSED [C, R], inv fp32 [R/128, C], scale fp32 [R/128, C]): 128 x 1 blocks."""
    x = _f32(xb)
    R, C = x.shape
    assert R % BLOCK == 0
    s = scale_of(np.abs(x).reshape(R // BLOCK, BLOCK, C).max(axis=1), clamp_in_bf16=True)
    return np.ascontiguousarray(_codes(x, np.repeat(s, BLOCK, axis=0)).T), _inv(s), s


def cast_weight(wb):
    """w bf16 bits [N, K] -> (codes uint8 [N, K], inv fp32 [N/128, K/128], scale fp32 [N/128, K/128]): 128 x 128 blocks."""
    w = _f32(wb)
    N, K = w.shape
    assert N % BLOCK == 0 and K % BLOCK == 0
    s = scale_of(np.abs(w).reshape(N // BLOCK, BLOCK, K // BLOCK, BLOCK).max(axis=(1, 3)))
    return _codes(w, np.repeat(np.repeat(s, BLOCK, axis=0), BLOCK, axis=1)), _inv(s), s


def dequant_rows(q, inv):
    return fp8_ref.e4m3_to_f32(q).astype(np.float64) * np.repeat(np.asarray(inv, dtype=np.float64), BLOCK, axis=1)


def dequant_cols(q_t, inv):
    """The [R, C] values of a column cast (codes [C, R], inv [R/128, C]), float64."""
    return fp8_ref.e4m3_to_f32(q_t).astype(np.float64).T * np.repeat(np.asarray(inv, dtype=np.float64), BLOCK, axis=0)


def dequant_weight(q, inv):
    return fp8_ref.e4m3_to_f32(q).astype(np.float64) * np.repeat(np.repeat(np.asarray(inv, dtype=np.float64), BLOCK, axis=0), BLOCK, axis=1)


def _token_blocks(g_t, x_t):
    g = fp8_ref.e4m3_to_f32(g_t).astype(np.float64)
    x = fp8_ref.e4m3_to_f32(x_t).astype(np.float64)
    assert g.shape[1] == x.shape[1] and g.shape[1] % BLOCK == 0
    return g, x, g.shape[1] // BLOCK


def wgrad_f64(g_t, g_inv, x_t, x_inv):
    """(y, S) [N, K] in float64 with the scales applied: y = sum_mb p_mb g_inv[mb][n] x_inv[mb][k]; S the same sum of absolute products
    (|g|^T |x|).  g_t codes [N, M], g_inv [M/128, N], x_t codes [K, M], x_inv [M/128, K]."""
    g, x, mb = _token_blocks(g_t, x_t)
    g_inv, x_inv = np.asarray(g_inv, dtype=np.float64), np.asarray(x_inv, dtype=np.float64)
    y = np.zeros((g.shape[0], x.shape[0]), dtype=np.float64)
    S = np.zeros_like(y)
    for i in range(mb):
        sl = slice(i * BLOCK, (i + 1) * BLOCK)
        w = g_inv[i][:, None] * x_inv[i][None, :]
        y += (g[:, sl] @ x[:, sl].T) * w
        S += (np.abs(g[:, sl]) @ np.abs(x[:, sl]).T) * np.abs(w)
    return y, S


def wgrad_chain_bits(g_t, g_inv, x_t, x_inv):
    """The fp32 chain in block order, bf16 bits [N, K].  p_mb is the float64 block sum rounded to fp32 (exact whenever the block's
    partial sums are exact in fp32, as in the exact-sum tests)."""
    g, x, mb = _token_blocks(g_t, x_t)
    g_inv, x_inv = np.asarray(g_inv, dtype=np.float32), np.asarray(x_inv, dtype=np.float32)
    acc = np.zeros((g.shape[0], x.shape[0]), dtype=np.float32)
    for i in range(mb):
        sl = slice(i * BLOCK, (i + 1) * BLOCK)
        p = (g[:, sl] @ x[:, sl].T).astype(np.float32)
        t = (p * g_inv[i][:, None]).astype(np.float32)
        u = (t * x_inv[i][None, :]).astype(np.float32)
        acc = (acc + u).astype(np.float32)
    return bf16.to_bits(bf16.bf16_round(acc))


def linear_emulation(xb, wb, gob):
    """(out [M, N], grad_input [M, K], grad_weight [N, K]) in float64 from the restatement's casts, every GEMM a float64 matmul of the
    dequantized operands: what the recipe computes with exact sums.  x bits [M, K], w bits [N, K], go bits [M, N]."""
    xq, xi, _ = cast_rows(xb)
    wq, wi, _ = cast_weight(wb)
    gq, gi, _ = cast_rows(gob)
    gt, gti, _ = cast_cols(gob)
    xt, xti, _ = cast_cols(xb)
    w = dequant_weight(wq, wi)
    return dequant_rows(xq, xi) @ w.T, dequant_rows(gq, gi) @ w, dequant_cols(gt, gti).T @ dequant_cols(xt, xti)
