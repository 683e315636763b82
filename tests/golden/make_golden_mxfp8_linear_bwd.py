"""Generate tests/golden/mxfp8_linear_bwd.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_mxfp8_linear_bwd.py

Everything runs on the CPU, through _to_mxfp8_then_scaled_mm(..., KernelPreference.EMULATED, mode, wgrad_with_hp)
(torchao/prototype/moe_training/mxfp8_linear.py:27-269) and out.backward(grad_out).  bf16 tensors are stored as uint16 bit patterns, codes
and E8M0 scales as uint8.

  x [2, 48, 288] (M = 96: three 32-token blocks, no multiple of 128), W [160, 288] (partial 128-tiles along N and K), go [2, 48, 160]
  x, w, go           the operands (randn, W * 0.05, go * 0.01: the grouped fixture's seeding and scaling)
  out_<v>, gi_<v>, gw_<v>   output [2, 48, N], grad_input [2, 48, K], grad_weight [N, K];  v: rceil_mx | rceil_hp | floor_mx
  go_q, go_s         to_mx(go [M, N]): codes [M, N], scales [M, N/32]         (RCEIL, like the three below)
  go_t_q, go_t_s     to_mx(go.t().contiguous()): codes [N, M], scales [N, M/32]
  x_t_q, x_t_s       to_mx(x.t().contiguous()):  codes [K, M], scales [K, M/32]
  w_t_q, w_t_s       to_mx(W.t().contiguous()):  codes [K, N], scales [K, N/32] -- the weight cast along N, the dgrad's operand

Tensors that come out with the same bits as an earlier one are stored once: the later key then holds a 0-d string naming the earlier key
(the output and the grad_input do not depend on wgrad_with_hp).  tests read them through `load()`.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "mxfp8_linear_bwd.npz")
B, T, N, K = 2, 48, 160, 288
VARIANTS = (("rceil_mx", "rceil", False), ("rceil_hp", "rceil", True), ("floor_mx", "floor", False))


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
    from torchao.prototype.moe_training.mxfp8_linear import _to_mxfp8_then_scaled_mm
    from torchao.prototype.mx_formats.config import ScaleCalculationMode
    from torchao.prototype.mx_formats.mx_tensor import to_mx
    from torchao.quantization.quantize_.common import KernelPreference

    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    go = (torch.randn(B, T, N, generator=g) * 0.01).to(torch.bfloat16)
    out = {"x": bits(x), "w": bits(w), "go": bits(go)}

    # fp32 matmuls of the unquantised tensors, for the SQNR printed below
    x2, go2 = x.reshape(-1, K).float(), go.reshape(-1, N).float()
    y32, gi32, gw32 = x2 @ w.float().t(), go2 @ w.float(), go2.t() @ x2

    stored = {}
    for tag, mode, hp in VARIANTS:
        x_ = x.clone().requires_grad_(True)
        w_ = w.clone().requires_grad_(True)
        y = _to_mxfp8_then_scaled_mm(x_, w_, KernelPreference.EMULATED, ScaleCalculationMode(mode), hp)
        y.backward(go)
        assert y.dtype == x_.grad.dtype == w_.grad.dtype == torch.bfloat16
        print("%-9s SQNR vs fp32: out %.2f dB, grad_input %.2f dB, grad_weight %.2f dB" % (
            tag, sqnr(y.reshape(-1, N), y32), sqnr(x_.grad.reshape(-1, K), gi32), sqnr(w_.grad, gw32)))
        for key, t in (("out_" + tag, bits(y)), ("gi_" + tag, bits(x_.grad)), ("gw_" + tag, bits(w_.grad))):
            same = next((k for k, v in stored.items() if v.shape == t.shape and np.array_equal(v, t)), None)
            if same is None:
                stored[key] = out[key] = t
            else:
                out[key] = np.array(same)
                print("  %s has the bits of %s" % (key, same))

    go2b, x2b = go.reshape(-1, N), x.reshape(-1, K)
    for name, t in (("go", go2b), ("go_t", go2b.t().contiguous()), ("x_t", x2b.t().contiguous()), ("w_t", w.t().contiguous())):
        s, q = to_mx(t, torch.float8_e4m3fn, 32, ScaleCalculationMode.RCEIL)
        out[name + "_q"], out[name + "_s"] = q.view(torch.uint8).numpy().copy(), s.view(torch.uint8).numpy().copy()

    np.savez_compressed(PATH, **out)
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
