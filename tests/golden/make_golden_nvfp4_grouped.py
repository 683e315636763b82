"""Generate tests/golden/nvfp4_grouped.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_nvfp4_grouped.py

Everything runs on the CPU.  bf16 tensors are stored as uint16 bit patterns, codes and e4m3 scales as uint8, per-expert scales as fp32.

  w3_*   NVFP4Tensor.to_nvfp4 of a 3-D bf16 weight [E = 3, N = 32, K = 80], is_swizzled_scales=False, with the per-expert scale
         per_tensor_amax_to_scale(amax(dim=(1, 2))).view(E, 1, 1) of inference_workflow.py:309-319 (w3_p_*) and without one (w3_nop_*):
         qdata, the scale bytes and dequantize(bf16)
  gw_*   the weight-only chain torch._grouped_mm(x, dequantize(bf16).transpose(-2, -1), offs) on exact-sum operands (integer x, |x| <= 8,
         any e2m1 codes, block scales in {1/4, 1/2, 1, 2}, per-expert scales that are powers of two and differ) for the group sizes
         gw_sizes, one of them empty; with the per-expert scale (gw_p_y) and without (gw_nop_y)
  ge_*   _emulated_nvfp4_scaled_grouped_mm_2d_3d (prototype/moe_training/nvfp4_grouped_mm.py:62-116) on activation codes from the
         reference's cast (nvfp4_quantize of ge_x, whose blocks are e2m1 values times 1 or 2 and so go through the cast unchanged)
         against the gw_ experts without a per-expert scale

torch._grouped_mm: where the installed torch has no CPU implementation the script records, per group, torch.mm of the SAME bf16 operands
(the rows of the group, the expert's transposed bf16 weight) instead, and says so on stdout and in the fixture's `grouped_mm_on_cpu` flag
(1: torch._grouped_mm ran; 0: the per-group torch.mm stand-in).
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def per_group_mm(a, b_t, offs):
    out = torch.zeros(a.shape[0], b_t.shape[-1], dtype=torch.bfloat16)
    start = 0
    for e, end in enumerate(offs.tolist()):
        if end > start:
            out[start:end] = torch.mm(a[start:end], b_t[e])
        start = end
    return out


def main():
    from torchao.prototype.moe_training import nvfp4_grouped_mm as ref_gmm
    from torchao.prototype.mx_formats.nvfp4_tensor import NVFP4Tensor, nvfp4_quantize, per_tensor_amax_to_scale

    g = torch.Generator().manual_seed(0)
    out = {}
    # ---- the 3-D cast
    E, N, K = 3, 32, 80
    w = (torch.randn(E, N, K, generator=g) * torch.tensor([0.02, 1.0, 37.0]).reshape(E, 1, 1)).to(torch.bfloat16)
    p = per_tensor_amax_to_scale(torch.amax(torch.abs(w), dim=(1, 2))).view(E, 1, 1)
    out["w3_w"], out["w3_p"] = bits(w), p.reshape(E).numpy().copy()
    for tag, pp in (("p", p), ("nop", None)):
        t = NVFP4Tensor.to_nvfp4(w, per_tensor_scale=pp, is_swizzled_scales=False)
        assert tuple(t.qdata.shape) == (E, N, K // 2) and tuple(t.scale.shape) == (E, N, K // 16)
        out[f"w3_{tag}_q"] = t.qdata.view(torch.uint8).numpy().copy()
        out[f"w3_{tag}_s"] = t.scale.view(torch.uint8).numpy().copy()
        out[f"w3_{tag}_deq"] = bits(t.dequantize(torch.bfloat16))
    # ---- the weight-only chain on exact-sum operands
    sizes = [5, 0, 17, 3]
    E, N, K = len(sizes), 24, 144
    offs = torch.tensor(sizes).cumsum(0).to(torch.int32)
    M = int(offs[-1])
    x = torch.randint(-8, 9, (M, K), generator=g).to(torch.bfloat16)
    codes = torch.randint(0, 256, (E, N, K // 2), generator=g).to(torch.uint8)
    scale = torch.exp2(torch.randint(-2, 2, (E, N, K // 16), generator=g).to(torch.float32)).to(torch.float8_e4m3fn)
    pe = torch.tensor([2.0 ** -3, 2.0 ** -1, 2.0 ** -2, 1.0], dtype=torch.float32).view(E, 1, 1)
    out["gw_sizes"], out["gw_x"], out["gw_q"] = np.asarray(sizes, dtype=np.int32), bits(x), codes.numpy().copy()
    out["gw_s"], out["gw_p"] = scale.view(torch.uint8).numpy().copy(), pe.reshape(E).numpy().copy()
    on_cpu = 1
    for tag, pp in (("p", pe), ("nop", None)):
        wt = NVFP4Tensor(codes, scale, 16, torch.bfloat16, pp)
        b_t = wt.dequantize(torch.bfloat16).transpose(-2, -1)
        try:
            y = torch._grouped_mm(x, b_t, offs)
        except (RuntimeError, NotImplementedError) as exc:
            print("torch._grouped_mm does not run on the CPU here (%s): recording per-group torch.mm of the same bf16 operands" % exc)
            on_cpu = 0
            y = per_group_mm(x, b_t, offs)
        assert torch.equal(y.view(torch.int16), per_group_mm(x, b_t, offs).view(torch.int16))  # exact sums: one rounding either way
        out[f"gw_{tag}_y"] = bits(y)
    # ---- the emulated codes x codes function on activation codes from the reference's cast
    vals = torch.tensor(E2M1)[torch.randint(0, 16, (M, K // 16, 16), generator=g)]
    vals[:, :, 5] = 6.0
    xa = (vals * torch.exp2(torch.randint(0, 2, (M, K // 16, 1), generator=g).to(torch.float32))).reshape(M, K).to(torch.bfloat16)
    a_s, a_q = nvfp4_quantize(xa, 16, None)
    a_s = a_s.view(M, K // 16)
    out["ge_x"], out["ge_aq"], out["ge_as"] = bits(xa), a_q.view(torch.uint8).numpy().copy(), a_s.view(torch.uint8).numpy().copy()
    try:
        y = ref_gmm._emulated_nvfp4_scaled_grouped_mm_2d_3d(a_q, a_s, codes, scale, offs)
    except (RuntimeError, NotImplementedError) as exc:
        print("_emulated_nvfp4_scaled_grouped_mm_2d_3d: torch._grouped_mm does not run on the CPU here (%s): its two dequantizations, "
              "then per-group torch.mm" % exc)
        on_cpu = 0
        a = ref_gmm._nvfp4_dequantize(a_q, a_s, 16, output_dtype=torch.bfloat16)
        b = ref_gmm._nvfp4_dequantize(codes, scale, 16, output_dtype=torch.bfloat16)
        y = per_group_mm(a, b.transpose(-2, -1), offs)
    out["ge_y"] = bits(y)
    out["grouped_mm_on_cpu"] = np.int32(on_cpu)
    np.savez_compressed(os.path.join(HERE, "nvfp4_grouped.npz"), **out)
    print({k: v.shape for k, v in out.items()}, "grouped_mm_on_cpu =", on_cpu)


if __name__ == "__main__":
    main()
