"""Generate tests/golden/mxfp8_grouped_bwd.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_mxfp8_bwd.py

Everything runs on the CPU, through _to_mxfp8_then_scaled_grouped_mm with KernelPreference.EMULATED
(torchao/prototype/moe_training/mxfp8_grouped_mm.py:56-316) and out.backward(grad_out).  bf16 tensors are stored as uint16 bit patterns,
codes and E8M0 scales as uint8.

  E = 3, N = 128, K = 256, group sizes [40, 0, 88]: a boundary inside a 32-token block, an empty expert.
  a, w, go, offs     A [M, K], W [E, N, K] (B_t = W.transpose(-2, -1)), grad_out [M, N], int32 cumulative ends
  out                the forward output [M, N]
  gi_<p>_<h>         grad_input [M, K];  gw_<p>_<h>  grad_weight [E, N, K] (W.grad)
                     p: nopad | pad (pad_token_groups_for_grouped_mm), h: mx | hp (wgrad_with_hp)
  go_t_q, go_t_s     to_mx(grad_out.t().contiguous()): codes [N, M], scales [N, M/32];  a_t_q, a_t_s the same of A.t()
  w_n_q, w_n_s       the weights cast along N (_quantize_3d_along_dim1_native, :864-895): codes [E, N, K], scales [E, N/32, K]

Gradients that come out with the same bits as an earlier one are stored once: the later key then holds a 0-d string naming the earlier key
(the grad_input does not depend on wgrad_with_hp, and rowwise casts do not see zero rows of padding).  tests read them through `load()`.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "mxfp8_grouped_bwd.npz")
E, N, K = 3, 128, 256
SIZES = [40, 0, 88]


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def load(path=PATH):
    """The fixture as a dict, aliases resolved."""
    z = np.load(path)
    out = {k: z[k] for k in z.files}
    for k, v in out.items():
        if v.dtype.kind == "U":
            out[k] = out[str(v)]
    return out


def sqnr(x, ref):
    return (10 * torch.log10(ref.double().pow(2).sum() / (x.double() - ref.double()).pow(2).sum())).item()


def main():
    from torchao.prototype.moe_training.mxfp8_grouped_mm import _quantize_3d_along_dim1_native, _to_mxfp8_then_scaled_grouped_mm
    from torchao.prototype.mx_formats.config import ScaleCalculationMode
    from torchao.prototype.mx_formats.mx_tensor import to_mx
    from torchao.quantization.quantize_.common import KernelPreference

    g = torch.Generator().manual_seed(0)
    M = sum(SIZES)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(E, N, K, generator=g) * 0.05).to(torch.bfloat16)
    go = (torch.randn(M, N, generator=g) * 0.01).to(torch.bfloat16)
    offs = torch.tensor(np.cumsum(SIZES), dtype=torch.int32)
    out = {"a": bits(a), "w": bits(w), "go": bits(go), "offs": offs.numpy().copy()}

    # fp32 matmuls of the unquantised tensors, for the SQNR printed below
    gi32, gw32, lo = torch.zeros(M, K), torch.zeros(E, N, K), 0
    for e, n in enumerate(SIZES):
        gi32[lo:lo + n] = go[lo:lo + n].float() @ w[e].float()
        gw32[e] = go[lo:lo + n].float().t() @ a[lo:lo + n].float()
        lo += n

    stored = {}
    for pad in (False, True):
        for hp in (False, True):
            a_ = a.clone().requires_grad_(True)
            w_ = w.clone().requires_grad_(True)
            y = _to_mxfp8_then_scaled_grouped_mm(a_, w_.transpose(-2, -1), offs, kernel_preference=KernelPreference.EMULATED, wgrad_with_hp=hp,
                                                 pad_token_groups_for_grouped_mm=pad)
            y.backward(go)
            assert y.dtype == a_.grad.dtype == w_.grad.dtype == torch.bfloat16
            assert not bool(w_.grad[1].any()), "the empty expert's slab must be zero"
            tag = "%s_%s" % ("pad" if pad else "nopad", "hp" if hp else "mx")
            print("%-9s SQNR vs fp32: grad_input %.2f dB, grad_weight %.2f dB" % (tag, sqnr(a_.grad, gi32), sqnr(w_.grad, gw32)))
            if not pad and not hp:
                out["out"] = bits(y)
            for key, t in (("gi_" + tag, bits(a_.grad)), ("gw_" + tag, bits(w_.grad))):
                same = next((k for k, v in stored.items() if v.shape == t.shape and np.array_equal(v, t)), None)
                if same is None:
                    stored[key] = out[key] = t
                else:
                    out[key] = np.array(same)
                    print("  %s has the bits of %s" % (key, same))

    for name, t in (("go_t", go), ("a_t", a)):
        s, q = to_mx(t.t().contiguous(), torch.float8_e4m3fn, 32, ScaleCalculationMode.RCEIL)
        out[name + "_q"], out[name + "_s"] = q.view(torch.uint8).numpy().copy(), s.view(torch.uint8).numpy().copy()
    q, s = _quantize_3d_along_dim1_native(w, 32, ScaleCalculationMode.RCEIL)
    out["w_n_q"], out["w_n_s"] = q.contiguous().view(torch.uint8).numpy().copy(), s.contiguous().view(torch.uint8).numpy().copy()
    assert out["w_n_q"].shape == (E, N, K) and out["w_n_s"].shape == (E, N // 32, K)

    np.savez_compressed(PATH, **out)
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
