"""Inputs of the GPTQ tests (tests/test_gptq_gpu.py), built on the CPU from fixed seeds.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import gptq_ref as R
from oracle import bf16

F32 = np.float32


def hinv(K, seed):
    """An upper-triangular fp32 [K, K] like the Cholesky factor gptq_quantize hands the kernel, made hard: the diagonal walks 2^-10 .. 2^4,
    row k's off-diagonal entries are its diagonal times N(0, 0.3) (so an error moves its neighbours by a fraction of itself, at any
    diagonal), and the lower triangle -- which a step never needs -- holds NaN: a kernel that used it would show."""
    rng = np.random.default_rng(seed)
    d = (2.0 ** ((np.arange(K) * 5) % 15 - 10)).astype(F32)
    h = (rng.standard_normal((K, K)).astype(F32) * F32(0.3) * d[:, None]).astype(F32)
    h[np.arange(K), np.arange(K)] = d
    h[np.tril_indices(K, -1)] = np.nan
    return h


def weights(N, K, g, is_bf16, seed):
    """[N, K] fp32 (bf16 values when is_bf16): Gaussian rows and, cyclically from row 1 on, rows that are hard for a group of g columns:
    1 every group all-equal (zero range: the int4 scale sits at its 1e-6 clamp);  2 all-zero;  3 values exactly on int4 rounding ties,
    (q + 1/2) scale + min built in fp32 from the group's own min / max;  4 one huge outlier a group;  0, 5, 6, ... Gaussian."""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((N, K)) * 0.5).astype(F32)
    if is_bf16:
        W = bf16.bf16_round(W)
    for r in range(N):
        kind = r % 7
        for g0 in range(0, K, g):
            if kind == 1:
                W[r, g0:g0 + g] = W[r, g0]
            elif kind == 2:
                W[r, g0:g0 + g] = 0
            elif kind == 3:
                mn, mx = F32(-1.0), F32(1.0 + (g0 // g) * 0.25)
                scale = (np.maximum(mx - mn, F32(1e-6)) / F32(15)).astype(F32)
                q = rng.integers(0, 15, size=g).astype(F32)
                v = ((q + F32(0.5)) * scale + mn).astype(F32)
                v[0], v[1] = mn, mx
                W[r, g0:g0 + g] = v  # (a bf16 weight keeps the fp32 construction only where it is representable: rounded below)
            elif kind == 4:
                W[r, g0 + 7 % g] = F32(300.0) * (1 if (g0 // g) % 2 == 0 else -1)
    return bf16.bf16_round(W) if is_bf16 else W


def aux_for(fmt, W, is_bf16):
    """NVFP4: a per-tensor scale taken from the GAUSSIAN rows only, so that the outlier rows' blocks saturate the e4m3 block scale at
    448 (the all-zero row gives zero groups);  int8: the row scales of the whole rows."""
    if fmt == R.NVFP4:
        return R.nvfp4_per_tensor_scale(W[0::7])
    if fmt == R.INT8:
        return R.int8_row_scale(W, is_bf16)
    return None


def e2e_inputs(out_features, seed=1234, in_features=256, batches=8, tokens=16, dead=7):
    """The end-to-end case: a bf16 weight [out, 256] and 8 batches of 16 x 256 bf16 activations x @ A with a fixed random A (correlated
    columns of unequal variance); input column `dead` is identically zero, so the Hessian has a dead column."""
    gen = torch.Generator().manual_seed(seed)
    A = torch.randn(in_features, in_features, generator=gen) / in_features ** 0.5 * torch.logspace(-0.5, 0.5, in_features)[None, :]
    xs = []
    for _ in range(batches):
        x = (torch.randn(tokens, in_features, generator=gen) @ A).to(torch.bfloat16)
        x[:, dead] = 0
        xs.append(x)
    # heavy-tailed, as trained weights are: two entries a row are 16 x larger, so a row's int8 step (amax / 127.5) is coarse next to the
    # bf16 rounding of the working matrix and GPTQ has an int8 error to remove
    W = torch.randn(out_features, in_features, generator=gen) * 0.05
    cols = torch.randint(0, in_features, (out_features, 2), generator=gen)
    W.scatter_(1, cols, W.gather(1, cols) * 16)
    return W.to(torch.bfloat16), xs


def identity_weight(out_features, seed=99, in_features=256):
    """The weight of the H = identity case: magnitudes in [0.25, 1] x 0.05 with random signs.  GPTQ under a diagonal Hessian is
    round-to-nearest, and byte for byte so where no value rounds to a zero code: a negative value that does keeps its sign in the e2m1
    code of the cast (-0, code 8), while GPTQ re-quantizes the column after its own update, where the residual w - err d has either
    sign.  Here every |w| is above 1 / 24 of its block's maximum, the smallest magnitude that still rounds to the code of 0.5."""
    gen = torch.Generator().manual_seed(seed)
    mag = 0.25 + 0.75 * torch.rand(out_features, in_features, generator=gen)
    sign = torch.randint(0, 2, (out_features, in_features), generator=gen) * 2 - 1
    return (mag * sign * 0.05).to(torch.bfloat16)


def hessian64(xs):
    """The running mean of observer.py:67-89 in float64: H = (2 / batches) sum X^T X, and the fp32-summation bound of computing it in fp32
    with one rescaling a batch: n 2^-23 (2 / tb) sum |x_i| |x_j|, n the tokens in all plus two roundings a batch."""
    tb, H, A = 0, None, None
    for x in xs:
        x2 = x.reshape(-1, x.shape[-1]).double().numpy()
        n = 1 if x.dim() == 2 else x.shape[0]
        H = (0 if H is None else H * (tb / (tb + n))) + (2.0 / (tb + n)) * (x2.T @ x2)
        A = (0 if A is None else A * (tb / (tb + n))) + (2.0 / (tb + n)) * (np.abs(x2).T @ np.abs(x2))
        tb += n
    terms = sum(x.reshape(-1, x.shape[-1]).shape[0] for x in xs) + 2 * len(xs)
    return H, terms * 2.0 ** -23 * A


def diag_hinv(K):
    """A DIAGONAL Hinv (2^-10 .. 2^4 on the diagonal, zeros above, NaN below): no error reaches another column, so every column meets
    the quantizer with the value the test gave it and under the qparams of the untouched group -- planted rounding ties stay ties."""
    h = np.zeros((K, K), F32)
    h[np.arange(K), np.arange(K)] = (2.0 ** ((np.arange(K) * 5) % 15 - 10)).astype(F32)
    h[np.tril_indices(K, -1)] = np.nan
    return h


E2M1_TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


def tie_weights(fmt, N, K, g, seed):
    """([N, K] weights exact in bf16 AND fp32, aux) whose every element but a group's two sentinels is a rounding tie of the format's
    quantizer, under qparams that are powers of two so that the quantizer's input is the tie exactly:
      int4   a group's sentinels -1 and 0.875 give scale = 1.875 / 15 = 2^-3, zero = 0, m = -1; the rest (q + 1/2) 2^-3 - 1, q = 0 .. 14
      int8   a row's sentinel 255 / 128 gives s = 2^-6; the rest +-(q + 1/2) 2^-6, q = 0 .. 126  (w (1 / s) = q + 1/2)
      NVFP4  p = 2^-10 (given); a block's sentinel 6 sf p with sf = 2^(b % 4) gives the e4m3 scale sf; the rest +-t sf p, t a midpoint
             between two e2m1 values (w r = t)
    Returns also how many elements are ties."""
    rng = np.random.default_rng(seed)
    W = np.zeros((N, K), F32)
    ties = 0
    if fmt == R.INT4:
        for g0 in range(0, K, g):
            q = rng.integers(0, 15, size=(N, g)).astype(F32)
            W[:, g0:g0 + g] = (q + F32(0.5)) * F32(0.125) - F32(1.0)
            W[:, g0 + 3], W[:, g0 + 9] = F32(-1.0), F32(0.875)
            ties += N * (g - 2)
        aux = None
    elif fmt == R.INT8:
        q = rng.integers(0, 127, size=(N, K)).astype(F32)
        W = ((q + F32(0.5)) * F32(2.0 ** -6) * rng.choice([-1, 1], size=(N, K)).astype(F32)).astype(F32)
        W[:, 5] = F32(255.0 / 128.0)
        ties = N * (K - 1)
        aux = R.int8_row_scale(W, True)
        assert np.all(aux == F32(2.0 ** -6))
    else:
        p = F32(2.0 ** -10)
        for b, g0 in enumerate(range(0, K, 16)):
            sf = F32(2.0 ** (b % 4))
            t = rng.choice(E2M1_TIES, size=(N, 16)).astype(F32) * rng.choice([-1, 1], size=(N, 16)).astype(F32)
            W[:, g0:g0 + 16] = t * sf * p
            W[:, g0 + 4] = F32(6.0) * sf * p
            ties += N * 15
        aux = p
    assert bf16.is_bf16(W)
    return W, aux, ties
