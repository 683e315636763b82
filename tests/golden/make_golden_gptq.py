"""Generate tests/golden/gptq.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_gptq.py

Everything runs on the CPU.  The reference's gptq_quantize itself cannot (prototype/gptq/api.py:390 asserts a CUDA device and the int4 branch
needs the un-vendored mslk package), so this maker drives the reference's importable pieces on torch CPU tensors in gptq_quantize's loop order
(api.py:392-532 and the final re-quantization :537-569):

  int4    _int4_row_quantize_zp_precomputed_qparams / _int4_row_dequantize_zp (api.py:167-221).  The group qparams are mslk's
          int4_row_quantize_zp in the reference; here the formula include/ao_mi355.h states for ao_int4_plain_quantize, in fp32 torch ops
          (PARITY UNPINNED, as in oracle/int4_plain_ref.py)
  NVFP4   nvfp4_quantize for the block scales, the uncompiled _nvfp4_with_precalculated_scales_qdq / _q, per_tensor_amax_to_scale
  int8    Int8Tensor.from_hp(scale=) + dequantize(float); the scale is from_hp's over the WHOLE row of the original weight (DESIGN.md
          records the deviation from api.py:471-478)
  H       GPTQObserverTensor._update_single_hessian on a few batches, one input column identically zero (a dead Hessian column)

bf16 tensors are stored as fp32 values (exact), e4m3 scales as bytes.  The file holds `cases` (a JSON list: name, fmt, bf16, N, K, B, g) and
per case <c>: <c>_H, <c>_W0, <c>_Hinv (fp32, after the dead columns, damping and the three Cholesky calls), <c>_aux (NVFP4: the per-tensor
scale; int8: the row scales), and per block b: <c>_b<b>_Win (W before the block), _Wstep (after its column loop), _Wout (after the lazy
batch update), _err, _qdata (the final codes of its columns), _scale, _zero (int4: fp32, before the rounding to W's dtype; NVFP4: bytes).

The maker asserts that tests/gptq_ref.py reproduces every recorded byte.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gptq_ref as R  # noqa: E402

from torchao.prototype.gptq import api as ref  # noqa: E402
from torchao.prototype.gptq.observer import GPTQObserverTensor  # noqa: E402
from torchao.prototype.mx_formats.nvfp4_tensor import nvfp4_quantize, per_tensor_amax_to_scale  # noqa: E402
from torchao.quantization import Int8Tensor  # noqa: E402
from torchao.quantization.granularity import PerRow  # noqa: E402

N, K, B, G = 3, 64, 32, 32
PERCDAMP = 0.01


def f32(t):
    return t.detach().to(torch.float32).contiguous().numpy().copy()


def hessian(gen):
    """four batches of 8 tokens, correlated columns of unequal variance, column 5 identically zero"""
    H = torch.zeros(K, K, dtype=torch.float32)
    tb = torch.zeros(1, dtype=torch.int64)
    A = torch.randn(K, K, generator=gen) * torch.logspace(-1, 1, K)[None, :]
    for _ in range(4):
        x = (torch.randn(8, K, generator=gen) @ A).to(torch.bfloat16)
        x[:, 5] = 0
        GPTQObserverTensor._update_single_hessian(x.float(), H, tb)
    return H


def int4_group_qparams(cols):
    x = cols.to(torch.float32)
    mx, mn = x.amax(dim=1), x.amin(dim=1)
    scale = torch.clamp(mx - mn, min=1e-6) / 15
    zero = mn + scale * 8
    return scale.reshape(1, -1), zero.reshape(1, -1)  # [1, N], the layout of mslk's outputs for one group


def run_case(fmt, is_bf16, gen):
    dtype = torch.bfloat16 if is_bf16 else torch.float32
    H = hessian(gen)
    W = (torch.randn(N, K, generator=gen) * 0.5).to(dtype)
    W[1, 40:56] = 0  # a zero NVFP4 block / part of an int4 group
    rec = {"H": f32(H), "W0": f32(W)}
    if fmt == R.NVFP4:
        p = per_tensor_amax_to_scale(torch.max(torch.abs(W)))
        rec["aux"] = f32(p)
    elif fmt == R.INT8:
        row_scale = Int8Tensor.from_hp(W, PerRow()).scale
        rec["aux"] = f32(row_scale).reshape(-1)
    H = H.clone()
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    W[:, dead] = 0
    damp = PERCDAMP * torch.mean(torch.diag(H))
    idx = torch.arange(K)
    H[idx, idx] += damp
    Hinv = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H)), upper=True)
    rec["Hinv"] = f32(Hinv)
    g = {R.INT4: G, R.NVFP4: 16, R.INT8: B}[fmt]
    for b, k0 in enumerate(range(0, K, B)):
        end = min(k0 + B, K)
        blk = W[:, k0:end]
        rec[f"b{b}_Win"] = f32(W)
        err = torch.zeros(N, end - k0, dtype=torch.float32)
        h = Hinv[k0:end, k0:end]
        scales, zeros = [], []
        for g0 in range(0, end - k0, g):
            cols = blk[:, g0:g0 + g]
            if fmt == R.INT4:
                scale, zero = int4_group_qparams(cols)
                scales.append(scale)
                zeros.append(zero)
            elif fmt == R.NVFP4:
                scale, _ = nvfp4_quantize(cols.contiguous(), per_tensor_scale=p)
                scales.append(scale)
            for k in range(g0, g0 + g):
                w = blk[:, k].unsqueeze(1)
                if fmt == R.INT4:
                    q = ref._int4_row_quantize_zp_precomputed_qparams(w, scale, zero, g)
                    dq = ref._int4_row_dequantize_zp(q, scale, zero, g)
                elif fmt == R.NVFP4:
                    dq = ref._nvfp4_with_precalculated_scales_qdq(w, p, scale.squeeze(-1))
                else:
                    dq = Int8Tensor.from_hp(w, granularity=PerRow(), scale=row_scale).dequantize(output_dtype=torch.float)
                e = (w - dq) / h[k, k]
                blk[:, k:] -= e.matmul(h[k, k:].unsqueeze(0))
                err[:, k] = e.flatten()
        rec[f"b{b}_Wstep"] = f32(W)
        rec[f"b{b}_err"] = f32(err)
        W[:, end:] -= err.matmul(Hinv[k0:end, end:])
        rec[f"b{b}_Wout"] = f32(W)
        # the final codes of the block's columns: what the re-quantization of the whole W (:537-569) gives for them, since later blocks never
        # touch these columns again
        if fmt == R.INT4:
            scale, zero = torch.cat(scales, dim=0), torch.cat(zeros, dim=0)
            q = ref._int4_row_quantize_zp_precomputed_qparams(blk, scale, zero, g)
            rec[f"b{b}_qdata"] = ((q.to(torch.int16)[:, 0::2] & 0xF) | ((q.to(torch.int16)[:, 1::2] & 0xF) << 4)).to(torch.uint8).numpy()  # pack_int4 (mslk): even k low
            rec[f"b{b}_scale"], rec[f"b{b}_zero"] = f32(scale), f32(zero)
        elif fmt == R.NVFP4:
            combined = torch.cat([s.reshape(1, N) for s in scales], dim=0).t().contiguous()
            rec[f"b{b}_qdata"] = ref._nvfp4_with_precalculated_scales_q(blk.contiguous(), p, combined).numpy().copy()
            rec[f"b{b}_scale"] = combined.view(torch.uint8).numpy().copy()
        else:
            rec[f"b{b}_qdata"] = Int8Tensor.from_hp(blk.contiguous(), granularity=PerRow(), scale=row_scale).qdata.numpy().copy()
    return rec


def check(name, fmt, is_bf16, rec):
    """tests/gptq_ref.py reproduces every recorded byte of the block steps"""
    g = {R.INT4: G, R.NVFP4: 16, R.INT8: 0}[fmt]
    aux = rec.get("aux")
    if fmt == R.NVFP4:
        assert R.nvfp4_per_tensor_scale(rec["W0"]) == aux.reshape(()), name
    elif fmt == R.INT8:
        assert np.array_equal(R.int8_row_scale(rec["W0"], is_bf16), aux), name
    for b, k0 in enumerate(range(0, K, B)):
        bw = min(B, K - k0)
        step = R.block_step(rec[f"b{b}_Win"], is_bf16, rec["Hinv"], k0, bw, fmt, g, None if aux is None else (aux.reshape(()) if fmt == R.NVFP4 else aux))
        for key, got in (("Wstep", step["W"]), ("err", step["err"]), ("qdata", step["qdata"]), ("scale", step.get("scale")), ("zero", step.get("zero"))):
            if f"b{b}_{key}" in rec:
                want = rec[f"b{b}_{key}"]
                assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (name, b, key)


def main():
    gen = torch.Generator().manual_seed(20260421)
    out, cases = {}, []
    for fmt in (R.INT4, R.INT8, R.NVFP4):
        for is_bf16 in (True, False):
            name = f"{fmt}_{'bf16' if is_bf16 else 'fp32'}"
            rec = run_case(fmt, is_bf16, gen)
            check(name, fmt, is_bf16, rec)
            cases.append({"name": name, "fmt": fmt, "bf16": is_bf16, "N": N, "K": K, "B": B, "g": {R.INT4: G, R.NVFP4: 16, R.INT8: 0}[fmt]})
            out.update({f"{name}_{k}": v for k, v in rec.items()})
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "gptq.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} cases, {os.path.getsize(path)} bytes; tests/gptq_ref.py reproduces every byte")


if __name__ == "__main__":
    main()
