"""numpy restatement of torchao's blockwise float8 MoE grouped-GEMM TRAINING op (prototype/moe_training/blockwise_fp8/grouped_mm.py).
TEST INFRASTRUCTURE ONLY.  The casts are those of tests/blockwise_fp8_training_ref.py (pinned byte for byte to the reference's torch
functions); this file adds the token groups: the padding of groups to 128 tokens, the three GEMMs per group as float64 products of the
dequantized casts, and the grouped weight gradient's fp32 chain.

  padding  prototype/moe_training/kernels/mxfp8/quant.py:368-430 (torch_pad_token_groups): group e moves to the next multiple of the
           alignment after group e - 1's padded end, inside a zero buffer of ceil((M + E a) / a) a rows; the group ends it returns are
           the padded ones, so every group is a whole number of 128-token blocks
  wgrad    grouped_mm_backend.py:158-194: the 128 x 1 casts of the WHOLE (padded) grad_output and A, block scales on the global 128-token
           grid, fed to a 2-D x 2-D grouped GEMM over offs.  Per (e, n, k), in fp32 (ao_fp8_block_grouped_mm_wgrad):
           acc = 0;  for every token block mb that meets the group, ascending: acc += (p * g_inv[mb][n]) * x_inv[mb][k], p the sum over
           the block's tokens INSIDE the group;  out = bf16(acc)

The fixture's operands are generated here (numpy's frozen legacy generator, whose streams never change) and pinned by their SHA-256 in
tests/golden/fp8_block_grouped_training.npz: the reference test's shapes (K = N = 256, M = 512 and 500) do not fit a committed file as
recorded tensors.  bf16 tensors are uint16 bit patterns, e4m3 codes uint8, scales float32.
"""
import hashlib

import numpy as np

import blockwise_fp8_training_ref as R
from blockwise_fp8_training_ref import bf16, fp8_ref  # noqa: F401

BLOCK = R.BLOCK
# the reference test's two cases (test/prototype/moe_training/test_fp8_blockwise_grouped_mm.py:37-43), K = N = 256
CASES = {"aligned": dict(offs=(256, 512), pad=False), "padded": dict(offs=(129, 384, 500), pad=True)}
N_FIX = K_FIX = 256
SAMPLE = 8  # the fixture keeps every 8th row of the reference's results


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def operands(case):
    """(A [M, K], W [E, N, K], grad_out [M, N]) as bf16 bits: randn, randn, 0.01 randn."""
    offs = CASES[case]["offs"]
    M, E = offs[-1], len(offs)
    g = np.random.RandomState(20 + len(offs))
    a = g.standard_normal((M, K_FIX)).astype(np.float32)
    w = g.standard_normal((E, N_FIX, K_FIX)).astype(np.float32)
    go = (g.standard_normal((M, N_FIX)) * 0.01).astype(np.float32)
    return tuple(bf16.to_bits(bf16.bf16_round(t)) for t in (a, w, go))


# ---- token groups ------------------------------------------------------------------------------------------------------------------------
def bounds(offs, M):
    """[(lo, hi)] per group: offs clamped to [0, M]; a non-increasing pair is an empty group (lo == hi)."""
    out, prev = [], 0
    for o in offs:
        lo, hi = min(max(int(prev), 0), M), min(max(int(o), 0), M)
        out.append((lo, hi) if hi > lo else (lo, lo))
        prev = o
    return out


def padded_offsets(offs, M, align=BLOCK):
    """(starts, ends, rows) of torch_pad_token_groups."""
    starts, ends, at, prev = [], [], 0, 0
    for o in offs:
        size = int(o) - prev
        starts.append(at)
        at += (size + align - 1) // align * align
        ends.append(at)  # the PADDED end: a group owns its zero rows
        prev = int(o)
    return np.array(starts, dtype=np.int32), np.array(ends, dtype=np.int32), (M + len(offs) * align + align - 1) // align * align


def pad_groups(xb, offs, align=BLOCK):
    """bits [M, C] -> (padded bits [rows, C], starts, ends); the padding is +0."""
    M = xb.shape[0]
    starts, ends, rows = padded_offsets(offs, M, align)
    out = np.zeros((rows, xb.shape[1]), dtype=xb.dtype)
    for (lo, hi), s in zip(bounds(offs, M), starts):
        out[s:s + hi - lo] = xb[lo:hi]
    return out, starts, ends


def unpad_groups(y, offs, starts, M):
    out = np.zeros((M,) + y.shape[1:], dtype=y.dtype)
    for (lo, hi), s in zip(bounds(offs, M), starts):
        out[lo:hi] = y[s:s + hi - lo]
    return out


# ---- the Function's casts and its three GEMMs as float64 products -------------------------------------------------------------------------
def function_casts(ab, wb, gob, offs, pad):
    """Every cast _Float8BlockwiseGroupedMM makes, by name: (codes, inv).  a_row / go_row [Mp, C]; a_col / go_col TRANSPOSED [C, Mp] with
    inv [Mp/128, C]; w [E, N, K] with inv [E, N/128, K/128]; w_t [E, K, N] with inv [E, K/128, N/128].  Also the group ends used."""
    if pad:
        ap, starts, ends = pad_groups(ab, offs)
        gp = pad_groups(gob, offs)[0]
    else:
        ap, gp, starts, ends = ab, gob, None, np.asarray(offs, dtype=np.int32)
    c = {"a_row": R.cast_rows(ap)[:2], "go_row": R.cast_rows(gp)[:2], "a_col": R.cast_cols(ap)[:2], "go_col": R.cast_cols(gp)[:2]}
    w = [R.cast_weight(wb[e])[:2] for e in range(wb.shape[0])]
    c["w"] = (np.stack([q for q, _ in w]), np.stack([i for _, i in w]))
    c["w_t"] = (np.ascontiguousarray(c["w"][0].transpose(0, 2, 1)), np.ascontiguousarray(c["w"][1].transpose(0, 2, 1)))
    return c, starts, ends


def function_f64(casts, offs, starts, ends, M):
    """(out [M, N], grad_A [M, K], grad_W [E, N, K]) in float64: per group, the exact products of the dequantized casts."""
    a, go = R.dequant_rows(*casts["a_row"]), R.dequant_rows(*casts["go_row"])
    ac, gc = R.dequant_cols(*casts["a_col"]), R.dequant_cols(*casts["go_col"])
    E, N, K = casts["w"][0].shape
    rows = a.shape[0]
    out, ga, gw = np.zeros((rows, N)), np.zeros((rows, K)), np.zeros((E, N, K))
    los = starts if starts is not None else [lo for lo, _ in bounds(offs, M)]
    for e in range(E):
        lo, hi = int(los[e]), int(ends[e])
        w = R.dequant_weight(casts["w"][0][e], casts["w"][1][e])
        out[lo:hi] = a[lo:hi] @ w.T
        ga[lo:hi] = go[lo:hi] @ w
        gw[e] = gc[lo:hi].T @ ac[lo:hi]
    if starts is not None:
        out, ga = unpad_groups(out, offs, starts, M), unpad_groups(ga, offs, starts, M)
    return out, ga, gw


def sqnr(y, ref):
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(10 * np.log10(np.sum(ref ** 2) / np.sum((y - ref) ** 2)))


def sample(t):
    """Every SAMPLE-th row of a result ([M, C], or [E, N, K] per expert)."""
    return np.ascontiguousarray(t[..., ::SAMPLE, :])


# ---- the grouped weight gradient ------------------------------------------------------------------------------------------------------------
def exact_operands(M, N, K, seed):
    """_exact_operands of tests/test_blockwise_fp8_training_gpu.py, restated: integer e4m3 codes |q| <= 15 and power-of-two reciprocals
    within 2^7 of one another, so that every partial sum, in any order and over any subset of the tokens, is exact in fp32."""
    g = np.random.default_rng(seed)
    mb = M // BLOCK
    g_t = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (N, M)).astype(np.float32))
    x_t = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (K, M)).astype(np.float32))
    g_inv = np.exp2(g.integers(-2, 2, (mb, N))).astype(np.float32)
    x_inv = np.exp2(g.integers(-2, 3, (mb, K))).astype(np.float32)
    _, S = R.wgrad_f64(g_t, g_inv, x_t, x_inv)
    assert S.max() / 2.0 ** -4 < 2.0 ** 24, "the sums of this case are not exact in fp32 in every order"
    assert g_inv.max() * x_inv.max() / (g_inv.min() * x_inv.min()) <= 2.0 ** 7
    assert len(np.unique(g_inv)) > 1 and len(np.unique(x_inv)) > 1
    return g_t, g_inv, x_t, x_inv


def masked(q_t, lo, hi):
    """codes [C, M] with every token outside [lo, hi) set to code 0"""
    out = np.zeros_like(q_t)
    out[:, lo:hi] = q_t[:, lo:hi]
    return out


def grouped_wgrad_chain_bits(g_t, g_inv, x_t, x_inv, offs):
    """bf16 bits [E, N, K]: the fp32 chain per group.  A block that does not meet the group adds (0 * g_inv) * x_inv = 0: the chain over
    all blocks of the masked codes is the chain over the group's blocks."""
    M = g_t.shape[1]
    return np.stack([R.wgrad_chain_bits(masked(g_t, lo, hi), g_inv, masked(x_t, lo, hi), x_inv) for lo, hi in bounds(offs, M)])


def grouped_wgrad_f64(g_t, g_inv, x_t, x_inv, offs):
    """[(y, S)] per group in float64 (R.wgrad_f64 on the masked codes)."""
    M = g_t.shape[1]
    return [R.wgrad_f64(masked(g_t, lo, hi), g_inv, masked(x_t, lo, hi), x_inv) for lo, hi in bounds(offs, M)]
