"""The NF4 contracts (ao_amd/csrc/quant_math.h "NF4") restated in numpy: plain fp32 operations, each rounded ONCE to bf16, nearest even
(TEST INFRASTRUCTURE ONLY).  tests/golden/make_golden_nf4.py asserts that this file gives the bytes of torchao's NF4Tensor on the CPU.

Arrays that "are bf16" are uint16 bit patterns at the interfaces and bf16-valued float32 inside (oracle/bf16.py).  The mean of the block
maxima is the one value of the format that depends on a summation order: it is always an ARGUMENT here (its bf16 bits), never computed.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import bf16  # noqa: E402

# nf4_tensor.py:666-684
TABLE = [-1.0000, -0.6962, -0.5251, -0.3949, -0.2844, -0.1848, -0.0911, 0.0000,
         0.0796, 0.1609, 0.2461, 0.3379, 0.4407, 0.5626, 0.7230, 1.0000]
TABLE_BF16 = bf16.bf16_round(np.array(TABLE, dtype=np.float32))


def bits(t):
    """a bf16 torch tensor -> its int16 bit patterns"""
    return t.contiguous().view(torch.int16)


def table_is_on_the_2_pow_minus_11_grid():
    v = TABLE_BF16.astype(np.float64) * 2048
    return bool(np.all(v == np.round(v)))


def block_absmax(x_bits, B):
    """max |x| per block of the flattened tensor (exact) -> bf16-valued float32 [numel / B]; NaN if the block holds one"""
    x = np.abs(bf16.from_bits(np.asarray(x_bits).reshape(-1, B)))
    a = x.max(axis=1)  # np.max propagates NaN
    return a.astype(np.float32)


def codes_of(v):
    """v bf16-valued float32 (any shape) -> uint8 codes: the FIRST index that minimises |bf16(v - table[i])|; a NaN v gives 0."""
    v = np.asarray(v, dtype=np.float32)
    best = np.zeros(v.shape, dtype=np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        bd = np.abs(bf16.bf16_round(v - TABLE_BF16[0]))
        for i in range(1, 16):
            d = np.abs(bf16.bf16_round(v - TABLE_BF16[i]))
            lt = d < bd  # False where either is NaN
            bd = np.where(lt, d, bd)
            best = np.where(lt, np.uint8(i), best)
    return best


def quantize(x_bits, B, SB, mean_bits):
    """The cast.  Returns (absmax bits [numel/B], codes uint8 [numel/2], scalers int8 [numel/B], factors bits [numel/(B SB)], m0 bool
    [numel/(B SB)]: the scaler blocks with m = 0, whose scalers the contract leaves at 0 and the reference undefined)."""
    x = bf16.from_bits(np.asarray(x_bits).reshape(-1, B))
    a = block_absmax(x_bits, B)
    mean = bf16.from_bits(np.asarray(mean_bits, dtype=np.uint16).reshape(()))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = bf16.sub(a, mean).reshape(-1, SB)
        m = np.abs(c).max(axis=1)
        qf = bf16.div(np.float32(256.0), bf16.mul(np.float32(2.0), m))
        p = bf16.mul(c, qf[:, None])
        q = np.where(np.isnan(p), np.float32(0.0), np.clip(np.rint(p), -128.0, 127.0)).astype(np.int8)  # np.rint: half to even
        v = bf16.div(x, a[:, None])
    code = codes_of(v).reshape(-1)
    packed = ((code[0::2] << 4) | code[1::2]).astype(np.uint8)
    return bf16.to_bits(a), packed, q.reshape(-1), bf16.to_bits(qf), m == 0


def scalers(q, qf_bits, mean_bits, SB):
    """dequantize's scaler per block -> bf16-valued float32 [numel / B]"""
    qf = bf16.from_bits(np.asarray(qf_bits))
    mean = bf16.from_bits(np.asarray(mean_bits, dtype=np.uint16).reshape(()))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = bf16.div(np.asarray(q).reshape(-1, SB).astype(np.float32), qf[:, None])
        return bf16.add(s, mean).reshape(-1)


def unpack(codes):
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1)
    return np.stack([codes >> 4, codes & 15], axis=1).reshape(-1)


def dequantize(codes, q, qf_bits, mean_bits, B, SB):
    """-> bf16 bits [numel]"""
    s = scalers(q, qf_bits, mean_bits, SB)
    t = TABLE_BF16[unpack(codes)].reshape(-1, B)
    with np.errstate(invalid="ignore", over="ignore"):
        return bf16.to_bits(bf16.mul(t, s[:, None]).reshape(-1))


def _bf(bits_np, shape):
    return torch.from_numpy(np.ascontiguousarray(bits_np).view(np.int16).copy()).view(torch.bfloat16).reshape(shape)


def weight(codes, q, qf_bits, mean_bits, B, SB, shape):
    """the dequantized weight as a bf16 torch tensor (CPU)"""
    return _bf(dequantize(codes, q, qf_bits, mean_bits, B, SB), shape)


def sums(x, w):
    """float64 sums and absolute sums of x [M, K] (bf16 torch) against w [N, K] (bf16 torch)"""
    xd, wd = x.cpu().double(), w.cpu().double()
    return xd @ wd.t(), xd.abs() @ wd.abs().t()


def chain(m):
    """the output chain on a sum: one rounding to bf16 (through fp32, as the accumulator)"""
    return m.to(torch.float32).to(torch.bfloat16)


def linear(x, w):
    """bf16(sum_k x w) from the float64 sum -- the kernel's bits wherever the fp32 accumulation is exact"""
    return chain(sums(x, w)[0])
