"""Inputs of the AWQ GPU tests, shared with nothing on the device: plain CPU tensors, the same bytes from a seed on every machine.
TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

from oracle import bf16


def weights(N, K, seed):
    """bf16 values as fp32 [N, K]: 0.05 N(0, 1) with a few outliers"""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((N, K)).astype(np.float32) * np.float32(0.05)
    W[rng.random((N, K)) < 0.01] *= np.float32(8)
    return bf16.bf16_round(W)


def scales(R, K, seed):
    """bf16 values as fp32 [R, K]: row 0 all ones (round-to-nearest), the others log-uniform over 2^-7 .. 2^7"""
    rng = np.random.default_rng(seed + 1000)
    S = bf16.bf16_round(np.exp2(rng.uniform(-7, 7, (R, K))).astype(np.float32))
    S[0] = 1
    return S


def corner_weights(g):
    """[8, 2 g]: groups whose quotients (ws - m) / s land on rounding ties, an all-equal group, an all-zero group, -0.0"""
    W = np.zeros((8, 2 * g), np.float32)
    ramp = np.arange(g, dtype=np.float32) % 16
    ties = ramp.copy()
    ties[2:15] += np.float32(0.5)                 # min 0, max 15: s = 1, quotients k + 0.5 round to even
    W[0, :g], W[0, g:] = ties, -ties
    W[1, :g], W[1, g:] = ties * np.float32(0.25), ties * np.float32(2 ** -9) - np.float32(3)
    W[2, :g], W[2, g:] = np.float32(0.03125), np.float32(-1.5)   # all-equal groups: the 1e-6 clamp
    W[3, g:] = ramp * np.float32(0.125)                           # an all-zero group beside a plain one
    W[4, :g] = np.where(np.arange(g) % 2 == 0, np.float32(-0.0), np.float32(0.0))  # only signed zeros
    W[4, g:] = np.where(np.arange(g) % 3 == 0, np.float32(-0.0), ramp * np.float32(0.5))
    W[5, :g], W[5, g:] = np.float32(1e-7), ramp * np.float32(1e-8)  # ranges below the clamp
    W[6] = bf16.bf16_round(np.random.default_rng(g).standard_normal(2 * g).astype(np.float32) * np.float32(100))
    W[7, :g] = np.where(np.arange(g) == 5, np.float32(7.0), np.float32(-0.0))
    return bf16.bf16_round(W)


def corner_scales(g, seed=0):
    """[6, 2 g]: ones; exact powers of two (ties stay ties); the 1e-4 clamp's value and large normalised values; 2^-7 and 2^7 alternating;
    log-uniform over 2^-7 .. 2^7; one constant power of two (ties stay ties, the qparams move)"""
    K = 2 * g
    rng = np.random.default_rng(seed + g)
    S = np.ones((6, K), np.float32)
    S[1] = np.exp2(rng.integers(-7, 8, K)).astype(np.float32)
    S[2] = np.where(np.arange(K) % 2 == 0, np.float32(1e-4), np.float32(100.0))
    S[3] = np.where(np.arange(K) % 2 == 0, np.float32(2 ** -7), np.float32(2 ** 7))
    S[4] = np.exp2(rng.uniform(-7, 7, K)).astype(np.float32)
    S[5] = np.float32(0.125)
    return bf16.bf16_round(S)


def calibration(N, K, rows, seed):
    """(W bf16 [N, K], X bf16 [rows, K]) torch CPU tensors: inputs with per-channel magnitudes exp(N(0, 1)), W ~ 0.05 N(0, 1)"""
    gen = torch.Generator().manual_seed(seed)
    mag = torch.exp(torch.randn(K, generator=gen))
    X = (torch.randn(rows, K, generator=gen) * mag).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=gen) * 0.05).to(torch.bfloat16)
    return W, X


def two_linear_model(seed):
    """(W1 [128, 256], X [320, 256], W2 [64, 128], b1, b2), bf16 CPU tensors, for Linear(256, 128) -> Linear(128, 64): the inputs have
    per-channel magnitudes, and so has the hidden activation, through the row magnitudes of W1"""
    W1, X = calibration(128, 256, 320, seed)
    gen = torch.Generator().manual_seed(seed + 77)
    W1 = (W1.float() * torch.exp(torch.randn(128, 1, generator=gen))).to(torch.bfloat16)
    W2 = (torch.randn(64, 128, generator=gen) * 0.05).to(torch.bfloat16)
    b1, b2 = (torch.randn(128, generator=gen) * 0.1).to(torch.bfloat16), (torch.randn(64, generator=gen) * 0.1).to(torch.bfloat16)
    return W1, X, W2, b1, b2


# (N, K, g, rows, seed): the seeds are chosen so that the float64 losses of the best and the second-best ratio are at least 1e-3 (relative)
# apart; test_search asserts that gap before anything else
SEARCH = [(48, 256, 32, 384, 3), (48, 256, 128, 384, 3), (33, 512, 64, 200, 0), (16, 512, 256, 512, 0)]
