"""numpy restatement of the AWQ scale search as ao_amd/prototype/awq runs it: the chain of csrc/awq_kernels.hip byte for byte, and the loss of
the reference's formula in float64.  TEST INFRASTRUCTURE ONLY.  Paths relative to the reference torchao tree; pinned against
tests/golden/awq.npz, which tests/golden/make_golden_awq.py writes by driving the reference's AWQObserver.

  chain   prototype/awq/core.py:78-80 with the PLAIN int4 quantizer (include/ao_mi355.h: ao_int4_plain_quantize; its stored weight is the one
          csrc/int4_plain_kernels.hip's header states).  Per ratio r, row n, group of g columns, every step ONE fp32 operation (numpy float32
          arithmetic is exactly that), IEEE division, rint to even:
            ws = bf16(W S[r]);  M, m = max, min over the group;  s = max(M - m, 1e-6) / 15;  z = m + 8 s
            q  = clamp(rint((ws - m) / s), 0, 15) - 8
            dq = bf16(bf16(q bf16(s)) + bf16(z))
            D  = W - dq / S[r]
  loss    core.py:81-83 without the bias (it cancels): mean((X W^T - (X / S[r]) dq^T)^2) = mean((X D[r]^T)^2), in float64 from the stored
          inputs; and the same number through the Gram matrix, tr(D G D^T) / (rows N), G = X^T X.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import bf16  # noqa: E402

F32 = np.float32


def chain(W, S, g):
    """W [N, K], S [R, K]: bf16 values held in fp32.  Returns a dict of [R, N, K] fp32 arrays: ws (the scaled weight), q (the codes, -8 .. 7),
    dq (the dequantized weight, bf16 values) and D; and scale, zero [R, N, K / g] (fp32, before the rounding to bf16 on store)."""
    W, S = np.asarray(W, F32), np.asarray(S, F32)
    n, k = W.shape
    r = S.shape[0]
    assert k % g == 0 and S.shape[1] == k and bf16.is_bf16(W) and bf16.is_bf16(S)
    ws = bf16.bf16_round((W[None] * S[:, None, :]).astype(F32))
    grp = ws.reshape(r, n, k // g, g)
    M, m = grp.max(axis=3), grp.min(axis=3)
    s = (np.maximum((M - m).astype(F32), F32(1e-6)) / F32(15)).astype(F32)
    z = (m + (s * F32(8)).astype(F32)).astype(F32)
    with np.errstate(over="ignore"):
        t = ((grp - m[..., None]).astype(F32) / s[..., None]).astype(F32)
    q = (np.clip(np.rint(t), F32(0), F32(15)) - F32(8)).astype(F32)
    sb, zb = bf16.bf16_round(s), bf16.bf16_round(z)
    p = bf16.bf16_round((q * sb[..., None]).astype(F32))
    dq = bf16.bf16_round((p + zb[..., None]).astype(F32)).reshape(r, n, k)
    D = (W[None] - (dq / S[:, None, :]).astype(F32)).astype(F32)
    return {"ws": ws, "q": q.reshape(r, n, k).astype(np.int8), "dq": dq, "D": D, "scale": s, "zero": z}


def scaled_error(W, S, g):
    """D fp32 [R, N, K], every fp32 rounding of ao_awq_scaled_error."""
    return chain(W, S, g)["D"]


def losses64(W, S, g, X):
    """float64 [R]: mean((X D[r]^T)^2) from the stored inputs X [rows, K] -- the reference's own formula on this library's D."""
    D = scaled_error(W, S, g).astype(np.float64)
    X = np.asarray(X, np.float64)
    return np.array([np.mean((X @ D[r].T) ** 2) for r in range(D.shape[0])])


def gram_losses64(W, S, g, X):
    """float64 [R]: tr(D[r] G D[r]^T) / (rows N), G = X^T X in float64."""
    D = scaled_error(W, S, g).astype(np.float64)
    X = np.asarray(X, np.float64)
    G = X.T @ X
    return np.array([np.sum((D[r] @ G) * D[r]) for r in range(D.shape[0])]) / (X.shape[0] * D.shape[1])
