"""Plain restatements of the BitNet b1.58 chains (csrc/bitnet_kernels.hip states them) in numpy float32 -- one IEEE operation a step, no
fused multiply-add -- with torch used only to round to bfloat16.  The matmul's sum is an int64 product: exact."""
import numpy as np
import torch

EPS = np.float32(1e-5)


def f32(t):
    return t.float().numpy()


def to_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16)


def absmean64(w):
    return float(np.abs(w.double().numpy()).mean())


def pack(q):
    """int8 [N, K] of 2-bit values -> int8 [N, K / 4]: k = 4j + s at bits 7 - 2s .. 6 - 2s of byte j."""
    u = (q.reshape(q.shape[0], -1, 4).astype(np.uint8) & 3).astype(np.uint32)
    return ((u[..., 0] << 6) | (u[..., 1] << 4) | (u[..., 2] << 2) | u[..., 3]).astype(np.uint8).view(np.int8)


def unpack(packed):
    """int8 [N, K / 4] -> int8 [N, K], each field sign-extended (-2 .. 1)."""
    b = packed.view(np.uint8).astype(np.int32)
    f = np.stack([(b >> s) & 3 for s in (6, 4, 2, 0)], axis=-1).reshape(packed.shape[0], -1)
    return np.where(f >= 2, f - 4, f).astype(np.int8)


def quantize_weight(w, scale):
    """bf16 w [N, K], an fp32 scale -> (ternary int8 [N, K], packed int8 [N, K / 4])."""
    q = np.clip(np.rint(f32(w) / np.maximum(np.float32(scale), EPS)), -1, 1).astype(np.int8)
    return q, pack(q)


def quantize_act(x):
    """bf16 x [M, K] -> (int8 [M, K], bf16 scales [M])."""
    xf = f32(x)
    scale = to_bf16(np.abs(xf).max(axis=1) / np.float32(127))
    inv = np.float32(1) / np.maximum(f32(scale), EPS)
    return np.clip(np.rint(xf * inv[:, None]), -128, 127).astype(np.int8), scale


def mm(a, q, row_scale, tensor_scale, bias=None):
    """int8 a [M, K], ternary int8 q [N, K], bf16 row_scale [M], a bf16 tensor_scale, bf16 bias [N] or None -> bf16 [M, N]."""
    acc = a.astype(np.int64) @ q.astype(np.int64).T
    out = to_bf16((acc.astype(np.float32) * f32(row_scale)[:, None]) * f32(tensor_scale.reshape(())))
    return out if bias is None else to_bf16(f32(out) + f32(bias)[None, :])


def linear(x, w, scale, bias=None):
    """The whole forward of one BitNet linear on bf16 x [M, K], bf16 w [N, K] under the fp32 abs-mean `scale`."""
    a, rs = quantize_act(x)
    q, _ = quantize_weight(w, scale)
    return mm(a, q, rs, to_bf16(np.float32(scale)), bias)
