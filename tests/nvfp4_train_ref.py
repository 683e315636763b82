"""torch-CPU restatement of the NVFP4 TRAINING contracts (csrc/quant_math.h "NVFP4 training").  TEST INFRASTRUCTURE ONLY.  Paths relative
to the reference torchao tree; pinned against tests/golden/nvfp4_training.npz, which tests/golden/make_golden_nvfp4_training.py writes from
the reference's own test/prototype/moe_training/nvfp4_training/nvfp4_reference.py.

  global  S_enc = min(2688 / amax, FLT_MAX), 1 if amax == 0 or the quotient is 0;  S_dec_global = 1 / S_enc
  block   s8 = e4m3(min(block_amax (S_enc (1/6)), 448)): no lower clamp
  encode  enc = min(1 / (f32(s8) S_dec_global), FLT_MAX);  scaled = clamp(x enc, -6, 6);  code = e2m1_rne(scaled) (nvfp4_ref.e2m1_codes)
  RHT     y_j = bf16(1/4 sum_i s_i a_i (-1)^popcount(i & j)) over 16 consecutive elements, the fp32 sum by the butterfly i ^ 1, i ^ 2, i ^ 4,
          i ^ 8 -- the kernel's order, so the bytes agree on any input; on inputs whose exponents span fewer than 12 binades every order
          gives the same sum
  SR      this library's own: a = min(|scaled|, 6), lo <= a <= hi its grid neighbours, t = (a - lo) / (hi - lo); up iff r16 < t 65536
  bits    Philox4x32-10, key = the halves of the int64 seed, counter = (g_lo, g_hi, offset & 0xFFFFFFFF, stream), g the row-major index of
          the group of 8 codes in the output, stream 0 the row and 1 the column output; element j takes bits 16 (j & 1) .. + 15 of word j >> 1
  GEMM    out = bf16(f32(sum_k (a_code a_s8)(b_code b_s8)) (pa pb)), the sum in float64 rounded to fp32 (_parity.oracle_round), ONE rounding
Every step is one fp32 torch operation.  NaN and Inf are outside the contract.
"""
import numpy as np
import torch

import nvfp4_ref as R

F32_MAX = torch.finfo(torch.float32).max
BLOCK = 16
DEFAULT_SIGN_VECTOR = (1, 1, 1, -1, 1, -1, -1, -1, -1, -1, -1, 1, -1, 1, -1, -1)
E2M1_GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _f32(v):
    return torch.as_tensor(v, dtype=torch.float32)


# ---- the randomized Hadamard transform and the amaxes -------------------------------------------------------------------------------------
def rht16(v, sign_vector=DEFAULT_SIGN_VECTOR):
    """[..., 16] fp32 -> [..., 16] bf16: the signs, four butterfly stages in fp32, x 1/4, one rounding."""
    a = v.to(torch.float32) * _f32(sign_vector)
    cols = list(a.unbind(-1))
    h = 1
    while h < 16:
        for i in range(16):
            if i & h == 0:
                u, w = cols[i], cols[i | h]
                cols[i], cols[i | h] = u + w, u - w
        h <<= 1
    return ((torch.stack(cols, dim=-1) + 0.0) * 0.25).to(torch.bfloat16)  # + 0: a sum of -0 terms alone is +0, as from an accumulator


def rht_t(x, sign_vector=DEFAULT_SIGN_VECTOR):
    """bf16 [M, N] -> bf16 [N, M] = RHT(x^T), the transform along M in runs of 16."""
    m, n = x.shape
    return rht16(x.t().reshape(n, m // BLOCK, BLOCK), sign_vector).reshape(n, m)


def amaxes(x, sign_vector=DEFAULT_SIGN_VECTOR, want_rht=True):
    """fp32 [2]: (max|RHT(x^T)| or 0, max|x|)"""
    col = rht_t(x, sign_vector).float().abs().max() if want_rht and x.numel() else _f32(0.0)
    row = x.float().abs().max() if x.numel() else _f32(0.0)
    return torch.stack([col, row])


# ---- the scale chain ------------------------------------------------------------------------------------------------------------------------
def global_scales(amax):
    amax = _f32(amax).reshape(())
    s_enc = torch.clamp(_f32(2688.0) / amax, max=F32_MAX)
    s_enc = torch.where((amax == 0) | (s_enc == 0), _f32(1.0), s_enc)
    return s_enc, _f32(1.0) / s_enc


def encode(block_amax, amax):
    """block amaxes fp32 [...] -> (scale bytes uint8 [...], encode scales fp32 [...])"""
    s_enc, s_dec = global_scales(amax)
    s8 = torch.clamp(block_amax * (s_enc * _f32(1.0 / 6.0)), max=448.0).to(torch.float8_e4m3fn)
    enc = torch.clamp(_f32(1.0) / (s8.to(torch.float32) * s_dec), max=F32_MAX)
    return s8.view(torch.uint8), enc


# ---- Philox4x32-10 and the stochastic rounding -----------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """uint64 numpy arrays holding 32-bit words -> the four output words"""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & m32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def random16(rows, cols, seed, offset, stream):
    """The 16 random bits of every element of a [rows, cols] output (cols a multiple of 8): int64 tensor."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & 0xFFFFFFFF
    g = np.arange(rows * cols // 8, dtype=np.uint64)
    with np.errstate(over="ignore"):
        words = philox4x32_10(g, g >> np.uint64(32), np.full_like(g, offset), np.full_like(g, stream), seed & 0xFFFFFFFF, seed >> 32)
    w = np.stack(words, axis=-1)                                            # [groups, 4]
    r = np.stack([w & np.uint64(0xFFFF), w >> np.uint64(16)], axis=-1)      # [groups, 4, 2]: element j = 2 word + half
    return torch.from_numpy(r.reshape(rows, cols).astype(np.int64))


def sr_codes(scaled, r16):
    """clamped fp32 values and their 16 random bits -> e2m1 codes (uint8), the sign bit kept"""
    a = scaled.abs().clamp(max=6.0)
    grid = _f32(E2M1_GRID)
    lo_c = (torch.searchsorted(grid, a.contiguous(), right=True) - 1).clamp(0, 7)
    hi_c = (lo_c + 1).clamp(max=7)
    lo, hi = grid[lo_c], grid[hi_c]
    step = torch.where(hi > lo, hi - lo, _f32(1.0))
    t = (a - lo) / step
    up = r16.to(torch.float32) < t * 65536.0
    c = torch.where(up, hi_c, lo_c).to(torch.uint8)
    return c | ((scaled.view(torch.int32) < 0).to(torch.uint8) * 8)


def pack(c):
    return (c[:, 0::2] | (c[:, 1::2] << 4)).contiguous()


# ---- the casts --------------------------------------------------------------------------------------------------------------------------------
def cast(v, amax, block_rows=1, sr=None):
    """bf16 / fp32 [R, C] under the per-tensor amax -> (codes uint8 [R, C/2], scale bytes uint8 [R, C/16]); block_rows 1 or 16 (the scale
    of a 16 x 16 block replicated over its rows); sr = (seed, offset, stream) or None for round to nearest even."""
    rows, cols = v.shape
    v = v.to(torch.float32)
    nr, nc = rows // block_rows, cols // BLOCK
    # one amax a block of block_rows x 16: the block's elements brought together on the last axis
    blocks = v.abs().reshape(nr, block_rows, nc, BLOCK).permute(0, 2, 1, 3).reshape(nr, nc, block_rows * BLOCK)
    s8, enc = encode(blocks.max(dim=-1).values, amax)
    # every element under its block's encode scale: [nr, 1, nc, 1] against [nr, block_rows, nc, 16]
    scaled = torch.clamp(v.reshape(nr, block_rows, nc, BLOCK) * enc.reshape(nr, 1, nc, 1), -6.0, 6.0).reshape(rows, cols)
    c = R.e2m1_codes(scaled) if sr is None else sr_codes(scaled, random16(rows, cols, *sr))
    return pack(c), s8.reshape(nr, 1, nc).expand(nr, block_rows, nc).reshape(rows, nc).contiguous()


def quantize_row_col(x, amax2, sign_vector=DEFAULT_SIGN_VECTOR, sr_seed=None, col_offset=0, row_offset=0):
    """(col_q [N, M/2], col_s [N, M/16], row_q [M, N/2], row_s [M, N/16])"""
    col = cast(rht_t(x, sign_vector), amax2[0], sr=None if sr_seed is None else (sr_seed, col_offset, 1))
    row = cast(x, amax2[1], sr=None if sr_seed is None else (sr_seed, row_offset, 0))
    return col + row


def quantize_weight_2d(w, amax):
    """(q [N, K/2], s [N, K/16], qt [K, N/2], st [K, N/16])"""
    return cast(w, amax, 16) + cast(w.t().contiguous(), amax, 16)


# ---- the GEMM and the linear -----------------------------------------------------------------------------------------------------------------
def scaled_mm_sums(a, a_s, b, b_s, pa, pb):
    """(ref64, S): acc (pa pb) with the sum over k in float64, and the same of absolute products; P is the fp32 product of the scales."""
    m, s = R.mm_sums(a, a_s, b, b_s)
    P = (_f32(pa).reshape(()) * _f32(pb).reshape(())).to(torch.float64)
    return m * P, s * P


def scaled_mm(a, a_s, b, b_s, pa, pb):
    m, _ = R.mm_sums(a, a_s, b, b_s)
    return (m.to(torch.float32) * (_f32(pa).reshape(()) * _f32(pb).reshape(()))).to(torch.bfloat16)


def amax_to_scale(amax):
    return _f32(amax) / 2688.0


def linear_sums(x, w, dy, sign_vector, sr_seed, col_offset, row_offset):
    """The three GEMMs of nvfp4_training.nvfp4_mm_hip restated on bf16 x [M, K], w [N, K], dy [M, N]: a dict of (ref64, S) for "out" (before
    the bias), "grad_input" and "grad_weight"."""
    xa, wa, da = amaxes(x, sign_vector), w.float().abs().max(), amaxes(dy, sign_vector)
    xcq, xcs, xrq, xrs = quantize_row_col(x, xa, sign_vector)
    wq, ws, wtq, wts = quantize_weight_2d(w, wa)
    dcq, dcs, drq, drs = quantize_row_col(dy, da, sign_vector, sr_seed, col_offset, row_offset)
    return {"out": scaled_mm_sums(xrq, xrs, wq, ws, amax_to_scale(xa[1]), amax_to_scale(wa)),
            "grad_input": scaled_mm_sums(drq, drs, wtq, wts, amax_to_scale(da[1]), amax_to_scale(wa)),
            "grad_weight": scaled_mm_sums(dcq, dcs, xcq, xcs, amax_to_scale(da[0]), amax_to_scale(xa[0]))}


def sqnr_db(got, want):
    got, want = got.detach().to(torch.float64), want.detach().to(torch.float64)
    return float(10.0 * torch.log10(want.pow(2).sum() / (got - want).pow(2).sum()))


def fp32_linear(x, w, dy):
    """out, grad_input, grad_weight of the fp32 matmuls on the bf16 operands"""
    xf, wf, df = x.float(), w.float(), dy.float()
    return {"out": xf @ wf.t(), "grad_input": df @ wf, "grad_weight": df.t() @ xf}
