"""numpy / CPU-torch restatement of GPTQ as ao_amd/prototype/gptq runs it: one block step (what csrc/gptq_kernels.hip computes, byte for
byte) and the whole gptq_quantize.  TEST INFRASTRUCTURE ONLY.  Paths relative to the reference torchao tree; pinned against
tests/golden/gptq.npz, which tests/golden/make_golden_gptq.py writes from the reference's importable pieces.

  loop         prototype/gptq/api.py:446-532.  For a block of columns [k0, k0 + bw) of W [N, K] (bf16 or fp32) and the upper Cholesky factor Hinv:
                 per group that starts in the block: qparams from the CURRENT values of its columns, then frozen
                 per column k:  dq = dequantize(quantize(w));  err = (w - dq) / Hinv[k, k];
                                W[:, k:k0+bw] -= err Hinv[k, k:k0+bw]  (rounded product, then the subtraction; a bf16 W rounds to bf16);  Err[:, k-k0] = err
                 codes of column k: quantize(its value after its own update), the frozen qparams (:537-569 computes the same)
               every step ONE fp32 operation (numpy float32 arithmetic is exactly that), IEEE division, rint to even
  int4         :167-221, qparams oracle.int4_plain_ref.quantize_zp kept in fp32 (PARITY UNPINNED: mslk is un-vendored):
               m = zero - 8 scale;  q = clamp(rint((w - m) / scale), 0, 15) - 8;  dq = (q + 8) scale + m
  NVFP4        :224-274, block scales tests/nvfp4_ref.cast under the per-tensor scale p:  r = (1 / p) / f32(s8);
               c = e2m1(clamp(w r, -6, 6));  dq = f32(c) / r
  int8         Int8Tensor.from_hp(scale=) + dequantize(float) (int8_tensor.py:176-259):  q = clamp(rint(w (1 / s)), -128, 127);  dq = q s,
               s the scale of the WHOLE row of the original weight (oracle.int8_ref.quantize_rowwise; the reference takes it from the first
               GPTQ block's columns, an accident of its loop: DESIGN.md)
  whole        :392-403 dead columns, damping, cholesky / cholesky_inverse / cholesky(upper) with torch on the CPU; per block the step above
               and W[:, end:] -= Err @ Hinv[k0:end, end:] (:530-532).  factor_dtype=float64 runs the factorization and the lazy update in
               float64 instead: the spread between the two is the only arithmetic the device path does not pin bit for bit.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nvfp4_ref  # noqa: E402
from oracle import bf16, int4_plain_ref, int8_ref  # noqa: E402

INT4, INT8, NVFP4 = "int4", "int8", "nvfp4"
F32 = np.float32
E2M1 = np.array(nvfp4_ref.E2M1_VALUES, dtype=np.float32)


def _round(w, is_bf16):
    return bf16.bf16_round(w) if is_bf16 else w.astype(F32)


def int8_row_scale(W, is_bf16):
    """The per-row scale of Int8Tensor.from_hp(W, PerRow()): amax / 127.5 in W's dtype, clamped at fp32 eps, as fp32."""
    W = np.asarray(W, F32)
    if is_bf16:
        return int8_ref.quantize_rowwise(W)[1]
    return np.maximum((np.abs(W).max(axis=1) / F32(127.5)).astype(F32), int8_ref.F32_EPS).astype(F32)


def nvfp4_per_tensor_scale(W):
    """per_tensor_amax_to_scale(max |W|): fp32 amax / 2688"""
    return F32(nvfp4_ref.amax_scale(torch.from_numpy(np.asarray(W, F32))).item())


class _Int4:
    def __init__(self, g):
        self.g = g

    def freeze(self, cols):
        _, s, z = int4_plain_ref.quantize_zp(cols, self.g)  # [1, N] each, fp32
        self.scale, self.zero = s[0], z[0]
        self.m = (self.zero - (self.scale * F32(8)).astype(F32)).astype(F32)
        return self.scale, self.zero

    def q(self, w):
        return (np.clip(np.rint(((w - self.m).astype(F32) / self.scale).astype(F32)), 0, 15) - 8).astype(np.int8)

    def dq(self, q):
        return (((q.astype(F32) + F32(8)) * self.scale).astype(F32) + self.m).astype(F32)


class _Nvfp4:
    g = 16

    def __init__(self, p):
        self.p = F32(p)

    def freeze(self, cols):
        _, s8 = nvfp4_ref.cast(torch.from_numpy(np.ascontiguousarray(cols)), torch.tensor(self.p, dtype=torch.float32))
        self.s8 = s8.numpy()[:, 0].copy()
        sf = torch.from_numpy(self.s8).view(torch.float8_e4m3fn).to(torch.float32).numpy()
        self.r = ((F32(1.0) / self.p).astype(F32) / sf).astype(F32)
        return self.s8, None

    def q(self, w):
        scaled = np.clip((w * self.r).astype(F32), F32(-6), F32(6))
        return nvfp4_ref.e2m1_codes(torch.from_numpy(scaled)).numpy()

    def dq(self, q):
        return (E2M1[q] / self.r).astype(F32)


class _Int8:
    def __init__(self, scale):
        self.scale = np.asarray(scale, F32)
        self.inv = (F32(1.0) / self.scale).astype(F32)

    def freeze(self, cols):
        return None, None

    def q(self, w):
        return np.clip(np.rint((w * self.inv).astype(F32)), -128, 127).astype(np.int8)

    def dq(self, q):
        return int8_ref.dequantize(q[:, None], self.scale)[:, 0].astype(F32)


def _format(fmt, g, aux):
    if fmt == INT4:
        return _Int4(g)
    if fmt == NVFP4:
        return _Nvfp4(aux)
    assert fmt == INT8
    return _Int8(aux)


def pack_nibbles(c):
    """[N, C] codes (low 4 bits used) -> [N, C/2] bytes, even column in the low nibble"""
    c = np.asarray(c).astype(np.uint8) & 0xF
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def block_step(W, is_bf16, Hinv, k0, bw, fmt, g=0, aux=None):
    """One GPTQ block on a COPY of W (fp32 array; bf16 values when is_bf16).  aux: NVFP4 the per-tensor scale, int8 the row scales [N].
    Returns dict: W (the whole matrix after the step), err [N, bw], codes [N, bw] (int4: q in -8..7, int8: q, NVFP4: e2m1 codes),
    qdata (int4 / NVFP4: packed [N, bw/2]; int8: codes), scale / zero (int4: fp32 [bw/g, N] BEFORE the rounding to W's dtype; NVFP4: scale
    bytes [N, bw/16])."""
    W = np.array(W, dtype=F32, copy=True)
    Hinv = np.asarray(Hinv, F32)
    n = W.shape[0]
    f = _format(fmt, g, aux)
    gsz = bw if fmt == INT8 else f.g
    assert bw % gsz == 0 and k0 % gsz == 0 and k0 + bw <= W.shape[1]
    err = np.zeros((n, bw), F32)
    codes = np.zeros((n, bw), np.int8 if fmt != NVFP4 else np.uint8)
    scales, zeros = [], []
    end = k0 + bw
    for g0 in range(k0, end, gsz):
        s, z = f.freeze(W[:, g0:g0 + gsz])
        scales.append(s)
        zeros.append(z)
        for k in range(g0, g0 + gsz):
            w = W[:, k].copy()
            e = ((w - f.dq(f.q(w))).astype(F32) / Hinv[k, k]).astype(F32)
            prod = (e[:, None] * Hinv[k, k:end][None, :]).astype(F32)
            W[:, k:end] = _round((W[:, k:end] - prod).astype(F32), is_bf16)
            err[:, k - k0] = e
            codes[:, k - k0] = f.q(W[:, k])
    out = {"W": W, "err": err, "codes": codes}
    if fmt == INT4:
        out["scale"], out["zero"] = np.stack(scales), np.stack(zeros)
        out["qdata"] = int4_plain_ref.pack_int4(codes)
    elif fmt == NVFP4:
        out["scale"] = np.stack(scales, axis=1)
        out["qdata"] = pack_nibbles(codes)
    else:
        out["qdata"] = codes
    return out


def factorize(H, W, percdamp=0.01, dtype=torch.float32):
    """api.py:392-403 on COPIES: dead columns, damping, the three Cholesky calls.  Returns (Hinv in `dtype` as numpy, W with its dead
    columns zeroed)."""
    H = torch.from_numpy(np.array(H, dtype=F32, copy=True)).to(dtype)
    W = np.array(W, dtype=F32, copy=True)
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    W[:, dead.numpy()] = 0
    damp = percdamp * torch.mean(torch.diag(H))
    idx = torch.arange(H.shape[0])
    H[idx, idx] += damp
    H = torch.linalg.cholesky(H)
    H = torch.cholesky_inverse(H)
    H = torch.linalg.cholesky(H, upper=True)
    return H.numpy(), W


def gptq_quantize(H, W, is_bf16, fmt, g=0, percdamp=0.01, block_size=256, factor_dtype=torch.float32, record=None):
    """The whole algorithm.  W: fp32 array (bf16 values when is_bf16).  Returns dict: qdata [N, K/2] (int8: [N, K]), W (the final working
    matrix), Hinv (fp32), and int4: scale / zero [K/g, N] rounded to W's dtype; NVFP4: scale bytes [N, K/16], p; int8: scale [N].
    record: a list that receives every block's step dict."""
    n, k = np.asarray(W).shape
    aux = None
    if fmt == NVFP4:
        aux = nvfp4_per_tensor_scale(W)
    elif fmt == INT8:
        aux = int8_row_scale(W, is_bf16)
    Hinv_f, W = factorize(H, W, percdamp, factor_dtype)
    Hinv = Hinv_f.astype(F32)
    qd, sc, zr = [], [], []
    for k0 in range(0, k, block_size):
        bw = min(block_size, k - k0)
        step = block_step(W, is_bf16, Hinv, k0, bw, fmt, g, aux)
        W = step["W"]
        end = k0 + bw
        if end < k:
            if factor_dtype == torch.float32:
                upd = torch.from_numpy(step["err"]).matmul(torch.from_numpy(np.ascontiguousarray(Hinv[k0:end, end:]))).numpy()
                W[:, end:] = _round((W[:, end:] - upd).astype(F32), is_bf16)
            else:
                upd = step["err"].astype(np.float64) @ Hinv_f[k0:end, end:].astype(np.float64)
                W[:, end:] = _round((W[:, end:].astype(np.float64) - upd).astype(F32), is_bf16)
        if record is not None:
            record.append(dict(step, W=W.copy()))
        qd.append(step["qdata"])
        sc.append(step.get("scale"))
        zr.append(step.get("zero"))
    out = {"qdata": np.concatenate(qd, axis=1), "W": W, "Hinv": Hinv}
    if fmt == INT4:
        out["scale"], out["zero"] = _round(np.concatenate(sc, axis=0), is_bf16), _round(np.concatenate(zr, axis=0), is_bf16)
    elif fmt == NVFP4:
        out["scale"], out["p"] = np.concatenate(sc, axis=1), aux
    else:
        out["scale"] = aux
    return out


def dequantize(res, fmt, g=0):
    """What the result stands for, in float64: the int4 / int8 formulas of the tensor classes in exact arithmetic on the stored fields;
    NVFP4: f32(code) (p f32(s8)) with the fp32 product of the scales, as NVFP4Tensor.dequantize."""
    if fmt == INT4:
        q = int4_plain_ref.unpack_int4(res["qdata"]).astype(np.float64)
        return q * np.repeat(res["scale"].T.astype(np.float64), g, axis=1) + np.repeat(res["zero"].T.astype(np.float64), g, axis=1)
    if fmt == INT8:
        return res["qdata"].astype(np.float64) * res["scale"].astype(np.float64)[:, None]
    codes = nvfp4_ref.unpack(torch.from_numpy(res["qdata"])).numpy()
    sf = torch.from_numpy(np.ascontiguousarray(res["scale"])).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    s32 = (F32(res["p"]) * sf).astype(F32)
    return E2M1[codes].astype(np.float64) * np.repeat(s32.astype(np.float64), 16, axis=1)


def objective(W, What, H):
    """L = tr((W - What) H (W - What)^T) in float64"""
    d = np.asarray(W, np.float64) - np.asarray(What, np.float64)
    return float(np.einsum("ij,jk,ik->", d, np.asarray(H, np.float64), d))
