"""Inputs and expected bytes of the training-cast edge tests (tests/test_training_casts_host.py and tests/test_training_casts_gpu.py).
TEST INFRASTRUCTURE ONLY: nothing here touches a kernel.  bf16 tensors are uint16 bit patterns; every expected byte comes from the
restatements the fixtures pin (fp8_training_ref, fp8_grouped_training_ref, blockwise_fp8_training_ref, nvfp4_train_ref, oracle.mx_ref).

  1. row casts     the case list of the one-launch row cast and the launcher's depth rule restated
  2. nvfp4 amax    matrices of more units than one trip of the amax grid, one large 16 x 2 unit planted
  3. amax -> scale matrices whose rows (blocks) have every non-negative finite bf16 as their amax
  4. value -> code the 65 536 bf16 patterns (NaN and Inf replaced by zero: non-finite inputs are outside the casts' contract, quant_math.h
                   "NaN and Inf inputs are outside the contract of the training casts") arranged so that every block is a maximum over the
                   binades below it
"""
import functools

import numpy as np
import torch

import blockwise_fp8_training_ref as B
import fp8_training_ref as R
import nvfp4_train_ref as T
from fp8_training_ref import bf16, fp8_ref
from oracle import mx_ref

SIGN = T.DEFAULT_SIGN_VECTOR


def f32(xb):
    return bf16.from_bits(np.asarray(xb, dtype=np.uint16)).astype(np.float32)


def t_bf16(xb):
    """uint16 bit patterns -> a torch bf16 tensor on the CPU"""
    return torch.from_numpy(np.ascontiguousarray(xb).view(np.int16).copy()).view(torch.bfloat16)


def bits_of(x_f32):
    """bf16-representable fp32 (numpy or torch) -> uint16 bit patterns"""
    if isinstance(x_f32, torch.Tensor):
        x_f32 = x_f32.float().numpy()
    u = np.ascontiguousarray(x_f32, dtype=np.float32).view(np.uint32)
    assert np.all((u & 0xFFFF) == 0)
    return (u >> 16).astype(np.uint16)


# ---- 1. the one-launch row cast --------------------------------------------------------------------------------------------------------------
# (2032: the ragged extent of depth 1, 254 of 256 threads hold a vector)
ROW_C = [2032, 2048, 2064, 4096, 4112, 8192, 8208, 16384, 16400, 32784]
ROW_R = [1, 3, 17]
ROW_THREADS = 256


def row_depth(C):
    """ao_fp8_train_quantize_rowwise's choice (fp8_train_kernels.hip:260-265): the register depth NV holding ceil(C / 8 / 256) 16-byte
    vectors a thread, 0 = the two-sweep form."""
    return next((nv for nv in (1, 2, 4, 8) if -(-(C // 8) // ROW_THREADS) <= nv), 0)


@functools.lru_cache(maxsize=None)
def row_case(R_, C, plant):
    """bf16 bits [R_, C]: every row its own magnitude 2^[-20, 20] (rows_of_many_magnitudes of test_quant_blocks_gpu.py), an all-zero row
    where R_ > 1, and the row's maximum (16 x its magnitude: Gaussian values stay below 8) planted ONCE, in the row's last 16-byte
    vector (`plant` = "last") or in its first ("first")."""
    g = torch.Generator().manual_seed(7 * C + R_)
    mag = torch.exp2(torch.randint(-20, 21, (R_, 1), generator=g).float())
    x = torch.randn(R_, C, generator=g).clamp(-7.5, 7.5) * mag
    col = C - 3 if plant == "last" else 5
    x[:, col] = (16.0 * mag[:, 0]) * torch.where(torch.arange(R_) % 2 == 0, 1.0, -1.0)
    if R_ > 1:
        x[R_ // 2] = 0
    return bits_of(x.to(torch.bfloat16))


# ---- 2. the NVFP4 amax past one trip of its grid ---------------------------------------------------------------------------------------------
AMAX_GRID_UNITS = 1024 * 256  # ao_nvfp4_train_amax (nvfp4_train_kernels.hip:259-261): at most 1024 workgroups of 256 threads, a unit a thread
AMAX_SHAPES = [(2048, 4096), (2064, 4096), (1040, 8080)]


def amax_units(m, n):
    return (m // 16) * (n // 2)


def amax_plants(m, n):
    """{name: (unit, sign)}: unit 0, the first unit of the second trip (where there is one) and the last unit of all."""
    units = amax_units(m, n)
    out = {"unit0": (0, 1.0), "last": (units - 1, -1.0)}
    if units > AMAX_GRID_UNITS:
        out["trip2"] = (AMAX_GRID_UNITS, 1.0)
    return out


@functools.lru_cache(maxsize=2)
def _amax_background(m, n):
    g = torch.Generator().manual_seed(m + n)
    return (torch.rand(m, n, generator=g) * 2.0 - 1.0).to(torch.bfloat16)  # |x| <= 1


def amax_case(m, n, plant):
    """(x bf16 [m, n] on the CPU, T.amaxes with the transform, T.amaxes without): |x| <= 1 but for one 16 x 2 unit (16 rows of a 16-row
    block x 2 adjacent columns, what one thread of the kernel reads) of values 50 .. 100 of both signs around one of +-200."""
    unit, sign = amax_plants(m, n)[plant]
    x = _amax_background(m, n).clone()
    half = n // 2
    mb, c2 = unit // half, unit % half
    g = torch.Generator().manual_seed(unit + 1)
    big = (50.0 + 50.0 * torch.rand(16, 2, generator=g)) * torch.where(torch.rand(16, 2, generator=g) < 0.5, -1.0, 1.0)
    big[5, 1] = 200.0 * sign
    x[16 * mb:16 * mb + 16, 2 * c2:2 * c2 + 2] = big.to(torch.bfloat16)
    return x, T.amaxes(x, SIGN, True), T.amaxes(x, SIGN, False)


def nvfp4_matrix(m, n, seed):
    """test_nvfp4_training_gpu._matrix: Gaussian values on per-run magnitudes with zeros, -0.0 and outliers."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, n, generator=g) * torch.exp2(torch.randint(-6, 7, (m // 16, 1), generator=g).float()).repeat_interleave(16, dim=0)
    x[torch.rand(m, n, generator=g) < 0.02] = 0.0
    x[torch.rand(m, n, generator=g) < 0.01] *= -0.0
    x[torch.rand(m, n, generator=g) < 0.01] *= 2.0 ** -14
    x[0, 0] = 300.0
    return x.to(torch.bfloat16)


NVFP4_CAST_SHAPE = (2064, 272)  # 17 x 3 tiles of 128 x 128
NVFP4_CAST_SR = (0x0123456789ABCDEF, 7, 7 ^ 0x5A5A)  # (seed, column offset, row offset)

# ---- 3. every amax -> scale ------------------------------------------------------------------------------------------------------------------
N_AMAX = 0x7F80  # the non-negative finite bf16 patterns 0x0000 .. 0x7F7F


def amax_rows(width):
    """bf16 bits [32640, width]: row i holds the pattern i once, as its amax (at column i % width, negative in every other run of
    `width` rows), and beside it zeros and SMALLER magnitudes of either sign (a non-negative bf16 orders like its bits: i - step)."""
    a = np.arange(N_AMAX, dtype=np.int64)[:, None]
    j = np.arange(width, dtype=np.int64)[None, :]
    step = 1 + (j * 37) % 251 + 128 * (j % 5)  # 1 .. 763: the same binade and several below it
    x = np.maximum(a - step, 0)
    x = np.where(j % 7 == 3, 0, x)
    x = x | np.where((j % 2 == 1) & (x > 0), 0x8000, 0)
    x[a[:, 0], a[:, 0] % width] = a[:, 0] | np.where((a[:, 0] // width) % 2 == 1, 0x8000, 0)
    return x.astype(np.uint16)


def amax_values():
    return f32(np.arange(N_AMAX, dtype=np.uint16))


def amax_groups():
    """(bf16 bits [32640, 16], offs int32 [2040]): 2 040 token groups of 16 rows over 16 columns; column c of group g has the amax
    16 g + c (the elements of amax_rows(16)'s row 16 g + c down the group's rows)."""
    x = amax_rows(16).reshape(N_AMAX // 16, 16, 16).transpose(0, 2, 1).reshape(N_AMAX, 16)
    return np.ascontiguousarray(x), (16 * np.arange(1, N_AMAX // 16 + 1)).astype(np.int32)


WEIGHT_MANTISSAS = (0, 1, 17, 42, 64, 96, 126, 127)


def weight_block_amaxes():
    """bf16 bits [2040]: every exponent 0 .. 254 x 8 mantissas"""
    e = np.arange(255, dtype=np.int64)[:, None]
    return ((e << 7) | np.asarray(WEIGHT_MANTISSAS, dtype=np.int64)[None, :]).reshape(-1).astype(np.uint16)


def weight_blocks():
    """bf16 bits [2040 * 128, 128]: block b (128 x 128) is zeros, five smaller values in its corners and middle, and its amax planted at
    (7 b % 128, 13 b % 128)."""
    a = weight_block_amaxes().astype(np.int64)
    nb = a.shape[0]
    w = np.zeros((nb, 128, 128), dtype=np.uint16)
    for k, (r, c) in enumerate(((0, 0), (127, 127), (0, 127), (127, 0), (64, 64))):
        v = np.maximum(a - (1 + 100 * k), 0)
        w[:, r, c] = v | np.where((v > 0) & (k % 2 == 1), 0x8000, 0)
    b = np.arange(nb)
    w[b, (7 * b) % 128, (13 * b) % 128] = a | np.where(b % 2 == 1, 0x8000, 0)
    return w.reshape(nb * 128, 128)


# per-tensor amaxes of the NVFP4 cast whose block amaxes are every value: the matrix's own (the largest bf16), a half and 2^-8 of it, 2688
# (S_enc = 1), 1 and the smallest normal bf16 (S_enc saturates at FLT_MAX)
NVFP4_TENSOR_AMAX_BITS = (0x7F7F, 0x7EFF, 0x7B7F, 0x4528, 0x3F80, 0x0080)


# ---- 4. every bf16 value -> code -------------------------------------------------------------------------------------------------------------
def finite(xb):
    """NaN and Inf patterns (exponent 255: 254 NaNs, +-Inf) replaced by zero"""
    xb = np.asarray(xb, dtype=np.uint16)
    return np.where((xb & 0x7F80) == 0x7F80, 0, xb).astype(np.uint16)


def all_values():
    """the 65 536 patterns in order, [256, 256]"""
    return finite(np.arange(65536, dtype=np.uint32).astype(np.uint16)).reshape(256, 256)


@functools.lru_cache(maxsize=None)
def blocks_over_binades(block, seed=0):
    """A permutation of the 65 536 patterns as [65536 / block, block]: the exponents are placed, the mantissas drawn.  Block (sign, E, g)
    holds `depth` = min(block, 32) binades, E at its head and E - d (mod 256) below it, block / depth values of each: the planted
    maximum and values from the binades below it, down to where an e4m3 or e2m1 cast flushes to zero.  The 128 mantissas of one (sign,
    exponent) are dealt by a seeded permutation over the 128 places the blocks E .. E + depth - 1 have for that exponent, so a value's
    mantissa is independent of its depth under the maximum.  (A block whose exponents wrap below 0, E < depth - 1, has its maximum near
    2^127 somewhere inside; exponent 255 is zeroed.)"""
    depth = min(block, 32)
    per, groups = block // depth, 128 // block
    rng = np.random.default_rng(seed)
    deal = np.stack([rng.permutation(128) for _ in range(512)]).reshape(2, 256, depth, groups, per)
    s, E, g, d, t = np.meshgrid(np.arange(2), np.arange(256), np.arange(groups), np.arange(depth), np.arange(per), indexing="ij")
    exp = (E - d) % 256
    pat = (s << 15) | (exp << 7) | deal[s, exp, d, g, t]
    pat = pat.transpose(1, 0, 2, 3, 4).reshape(-1, block)  # blocks in the order (E, sign, g)
    assert np.array_equal(np.sort(pat.reshape(-1)), np.arange(65536))
    return finite(pat.astype(np.uint16))


def row_blocks(block):
    """[256, 256]: every run of `block` consecutive elements of a row is one block of blocks_over_binades"""
    return blocks_over_binades(block).reshape(256, 256)


def col_blocks(block):
    """[256, 256]: every run of `block` consecutive elements of a COLUMN is one block"""
    return np.ascontiguousarray(blocks_over_binades(block).reshape(256 // block, 256, block).transpose(0, 2, 1).reshape(256, 256))


def weight_quadrants():
    """[256, 256]: the 128 x 128 block q holds both signs of about 64 binades, its maximum and everything below it down to the next
    block's.  The magnitudes 0 .. 32767 (a non-negative bf16 orders like its bits) are cut at 8192 + 40, 16384 - 77 and 24576 + 97 for
    the positive values and at 8192 - 40, 16384 + 77, 24576 - 97 for the negative ones, so each block has 16 384 values and the blocks'
    amaxes (positive, negative, positive, both) have the mantissas 39, 76, 96 and 127: 1.75 2^e (mantissa 96) makes the scale a power of two, where bf16 values sit on e4m3 ties; under the
    amaxes of mantissa 39 and 76, f32(amax) * f32(448 / amax) rounds ABOVE 448, which the clamp has to catch."""
    off = np.array([0, 40, -77, 97, 0])
    pos, neg = 8192 * np.arange(5) + off, 8192 * np.arange(5) - off
    blocks = []
    for k in range(4):
        vals = np.concatenate([np.arange(pos[k], pos[k + 1]), np.arange(neg[k], neg[k + 1]) | 0x8000])
        assert vals.shape == (16384,)
        blocks.append(vals[(np.arange(16384) * 5003) % 16384])        # spread over the block (5003 is odd: a permutation)
    q = np.stack(blocks).reshape(2, 2, 128, 128).transpose(0, 2, 1, 3).reshape(256, 256)
    assert np.array_equal(np.sort(q.reshape(-1)), np.arange(65536))
    return finite(q.astype(np.uint16))


E4M3_FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)  # 254 codes
_E4M3_MIDS = ((fp8_ref._POS[:-1].astype(np.float64) + fp8_ref._POS[1:].astype(np.float64)) / 2.0)
_E2M1_MIDS = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])


def e4m3_ties(t):
    """which fp32 values the e4m3 rounding meets exactly half way between two codes"""
    return np.isin(np.abs(np.asarray(t, dtype=np.float32)).astype(np.float64), _E4M3_MIDS)


def e2m1_ties(t):
    return np.isin(np.abs(np.asarray(t, dtype=np.float32)).astype(np.float64), _E2M1_MIDS)


BF16_MAX = float(f32(np.array([0x7F7F], dtype=np.uint16))[0])  # 3.39e38
# the amaxes GIVEN to the casts that take one, fp32: the matrix's own (the largest bf16), a quarter of it (the top binades saturate), and
# 448 2^k -- the scale is then 2^-k exactly, so bf16 values (8 significant bits) sit exactly half way between e4m3 codes (4 bits) and
# exactly on and above 448
FP8_GIVEN_AMAX = [BF16_MAX, BF16_MAX / 4.0, 448.0, 448.0 * 2.0 ** -20, 448.0 * 2.0 ** 100, 1.0]
# NVFP4: 2688 2^k makes S_enc = 2^-k; the block scales that are powers of two then put bf16 values on e2m1 ties and on the 6 clamp
NVFP4_GIVEN_AMAX = [BF16_MAX, BF16_MAX / 4.0, 2688.0, 2688.0 * 2.0 ** -20, 2688.0 * 2.0 ** 100]
NVFP4_VALUES_SR = (-5, 2 ** 32 - 1, 12345)


def fp8_given(xb, amax, pow2):
    """(codes [R, C], scale [], the fp32 products before the clamp) of the tensorwise cast under a given amax"""
    q, s, _ = R.cast_under(xb, np.float32(amax), pow2)
    with np.errstate(over="ignore"):
        return q, s, (f32(xb) * s).astype(np.float32)


def fp8_rowwise(xb, pow2):
    q, s, inv = R.cast(xb, -1, pow2)
    return q, s, inv, (f32(xb) * s).astype(np.float32)


def block_rows(xb):
    q, inv, s = B.cast_rows(xb)
    return q, inv, (f32(xb) * np.repeat(s, 128, axis=1)).astype(np.float32)


def block_cols(xb):
    q_t, inv, s = B.cast_cols(xb)
    return q_t, inv, (f32(xb) * np.repeat(s, 128, axis=0)).astype(np.float32)


def block_weight(wb):
    q, inv, s = B.cast_weight(wb)
    return q, inv, (f32(wb) * np.repeat(np.repeat(s, 128, axis=0), 128, axis=1)).astype(np.float32)


def mx_rows(xb, mode):
    """(codes [R, C], e8m0 [R, C/32], the fp32 products)"""
    x = f32(xb)
    q, e = mx_ref.to_mx(x, mode)
    return q, e, (x * np.repeat(mx_ref.e8m0_reciprocal_f32(e.reshape(-1)).reshape(e.shape), 32, axis=1)).astype(np.float32)


def mx_cols(xb, mode):
    """(codes transposed [C, R], e8m0 [R/32, C], the fp32 products [C, R]): the column cast is the row cast of the transpose"""
    q, e, t = mx_rows(np.ascontiguousarray(np.asarray(xb).T), mode)
    return q, np.ascontiguousarray(e.T), t


def nvfp4_rows(xb, amax, sr=None):
    """(codes [R, C/2], scale bytes [R, C/16], the fp32 products before the clamp) of the 1 x 16 cast of x itself under the per-tensor amax"""
    x = t_bf16(xb)
    q, s = T.cast(x, amax, sr=None if sr is None else (sr[0], sr[2], 0))
    v = x.float()
    _, enc = T.encode(v.abs().reshape(v.shape[0], -1, 16).max(dim=-1).values, amax)
    return q, s, (v.reshape(v.shape[0], -1, 16) * enc[..., None]).reshape(v.shape)


def unpack4(q):
    q = np.asarray(q, dtype=np.uint8)
    return np.stack([q & 0xF, q >> 4], axis=-1).reshape(q.shape[0], -1)
