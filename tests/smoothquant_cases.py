"""Inputs of the SmoothQuant tests, shared with nothing on the device: plain numpy arrays (bf16 values held in fp32), the same bytes from a seed
on every machine.  TEST INFRASTRUCTURE ONLY.

Columns and rows with a role, by index (so that K = 8 has every column role and every 97 columns have them again):
  column j % 97 == 0   pre = 1.5 and x = +-(1 + 2^-7) on even rows: the product 1.5 + 1.5 * 2^-7 lies exactly halfway between two bf16 values
  column j % 97 == 1   pre = 1 exactly
  column j % 97 == 2   pre = 2^-6;  j % 97 == 3: pre = 2^6.  Rows r % 5 == 1 hold 8 m in column 2 and m in column 3, m the row's largest
                       magnitude: column 2 carries the row's amax before scaling, column 3 after
  column j % 97 == 5   rows (r + seed) % 7 == 3 hold +-BIG, the largest finite bf16 whose product with 2^6 (and quotient by 2^-6) is finite
  column j % 13 == 6   rows (r + seed) % 7 == 5 hold bf16 subnormals, +-2^-130 and +-2^-133
  column j % 11 == 4   one row holds MINUS twice the column's largest magnitude: a negative carries the column's absmax
  column j % 29 == 7   only +0.0 and -0.0
and 2 % of everything else is +-0.0.  M = 1 and M = 2 have fewer of the row roles; the seeds of the tests move them."""
import numpy as np

from oracle import bf16

F32 = np.float32
BIG = F32(2.0 ** 121 * 1.9921875)  # bf16 max / 2^6
TIE = F32(1.0 + 2.0 ** -7)


def pre_scale(K, seed):
    """bf16 [K] as fp32: log-uniform over [2^-6, 2^6], a quarter exact ones, and the role columns above"""
    rng = np.random.default_rng(seed + 17)
    p = np.exp2(rng.uniform(-6, 6, K)).astype(F32)
    p[rng.random(K) < 0.25] = 1
    j = np.arange(K) % 97
    p[j == 0], p[j == 1], p[j == 2], p[j == 3] = 1.5, 1, 2.0 ** -6, 2.0 ** 6
    return bf16.bf16_round(p)


def smoothing_vector(K, seed):
    """bf16 [K] as fp32, positive: a divisor for the smoothed amax (kernel B): the same distribution as pre_scale"""
    return pre_scale(K, seed + 5)


def activation(M, K, seed, scale=1.0, big=True):
    """bf16 [M, K] as fp32: N(0, 1) with per-channel magnitudes exp(N(0, 1.5)) (activation outliers) times `scale`, and the roles above
    (big=False: without the +-BIG entries, which would be all that an amax over the whole tensor sees)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K)).astype(F32) * np.exp(rng.normal(0, 1.5, K)).astype(F32) * F32(scale)
    x = bf16.bf16_round(x)
    zero = rng.random((M, K)) < 0.02
    x[zero] = np.where(rng.random(int(zero.sum())) < 0.5, F32(-0.0), F32(0.0))
    rows, cols = np.arange(M), np.arange(K)
    j = cols % 97
    sign = np.where((rows[:, None] + cols[None, :]) % 2 == 0, F32(1), F32(-1))
    # a negative carries the column's absmax
    for c in cols[cols % 11 == 4]:
        x[c % M, c] = -F32(2) * np.abs(x[:, c]).max() - F32(scale)
    # the row's amax moves from column 2 to column 3 under the pre-scale
    if K > 3:
        for r in rows[rows % 5 == 1]:
            m = np.abs(x[r]).max() + F32(scale)
            x[r, j == 2], x[r, j == 3] = F32(8) * m, -m
    x = bf16.bf16_round(x)
    # ties of the product, on even rows
    x[::2, j == 0] = (TIE * sign)[::2][:, j == 0]
    big_rows, sub_rows = (rows + seed) % 7 == 3, (rows + seed) % 7 == 5
    if big:
        x[np.ix_(big_rows, j == 5)] = (BIG * sign)[np.ix_(big_rows, j == 5)]
    sub = np.where(cols % 2 == 0, F32(2.0 ** -130), F32(2.0 ** -133))[None, :] * sign
    x[np.ix_(sub_rows, cols % 13 == 6)] = sub[np.ix_(sub_rows, cols % 13 == 6)]
    x[:, cols % 29 == 7] = np.where(sign[:, cols % 29 == 7] > 0, F32(0.0), F32(-0.0))
    assert bf16.is_bf16(x) and np.isfinite(x).all()
    return x


def weight(N, K, seed):
    """bf16 [N, K] as fp32: 0.05 N(0, 1), a few outliers, one all-zero column (its absmax is 0: the eps of the smoothing factor)"""
    rng = np.random.default_rng(seed + 1000)
    W = rng.standard_normal((N, K)).astype(F32) * F32(0.05)
    W[rng.random((N, K)) < 0.01] *= F32(8)
    W[:, K // 3] = 0
    return bf16.bf16_round(W)


def toy_inputs(seed, batch=16, seq=10, k=512):
    """The reference accuracy test's input (test/prototype/test_smoothquant.py:40-59): randn [16, 10, 512] with 51 random channels times 10,
    as a bf16 torch CPU tensor from a seeded generator"""
    import torch

    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, seq, k, generator=gen).to(torch.bfloat16)
    n_outliers = max(1, int(k * 0.1))
    idx = torch.randperm(k, generator=gen)[:n_outliers]
    x[:, :, idx] *= 10.0
    return x


def toy_weights(seed):
    """The reference toy model's three bias-free linears 512 -> 256 -> 128 -> 64 (nn.Linear's default init), bf16 CPU tensors"""
    import torch

    gen = torch.Generator().manual_seed(seed + 4242)
    out = []
    for k, n in ((512, 256), (256, 128), (128, 64)):
        bound = 1.0 / k ** 0.5  # kaiming_uniform_(a = sqrt(5)) on [n, k]
        out.append(((torch.rand(n, k, generator=gen) * 2 - 1) * bound).to(torch.bfloat16))
    return out
