"""Generate tests/golden/fp8_training.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_fp8_training.py

Everything runs on the CPU.  bf16 tensors are stored as uint16 bit patterns, e4m3 codes as uint8, scales as float32.

  x [2, 40, 272], w [144, 272], go [2, 40, 144]   the operands (randn, W * 0.05, go * 0.01): M = 80, N = 144, K = 272, multiples of 16 and
                     of neither 64 nor 128, so every tile edge of the casts is partial
  edge [80, 48]      one all-zero row, one all-zero column, one row holding the largest finite bf16, one entry of 1e-20
  <t>_<a><p>_q, _s   hp_tensor_to_float8_dynamic (float8/float8_scaling_utils.py:29-72) of t in (x [80, 272], go [80, 144], w, edge):
                     a = r: AXISWISE along dim -1 (scale [R, 1]);  c: AXISWISE along dim 0 (scale [1, C]);  t: TENSORWISE (scale []);
                     p = 1 with round_scales_to_power_of_2, else 0.  Codes [R, C] in the tensor's own layout.
  out_<v>, gi_<v>, gw_<v>   output [2, 40, N], grad_input [2, 40, K], grad_weight [N, K] of Float8Linear.from_float(linear, config) with
                     emulate=True and out.backward(go);  v: rowwise | rowwise_with_gw_hp | tensorwise_e4m3 (the default config with
                     grad_output cast to e4m3)
  recipes            JSON: the fields of Float8LinearConfig.from_recipe_name(name) for the three names (`config_fields`)

The recorder asserts that every power-of-two scale it records equals the plain scale with its mantissa bits cleared, and that all codes
are finite.  Tensors that come out with the same bits as an earlier one are stored once: the later key then holds a 0-d string naming the
earlier key.  Tests read them through `load()`.
"""
import dataclasses
import enum
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fp8_training.npz")
B, T, N, K = 2, 40, 144, 272
RECIPES = ("tensorwise", "rowwise", "rowwise_with_gw_hp")
RUNS = ("rowwise", "rowwise_with_gw_hp", "tensorwise_e4m3")
AXES = (("r", -1), ("c", 0), ("t", None))


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def load(path=PATH):
    """The fixture as a dict, aliases resolved."""
    z = np.load(path)
    out = {k: z[k] for k in z.files}
    for k, v in out.items():
        if v.dtype.kind == "U" and k != "recipes":
            out[k] = out[str(v)]
    return out


def config_fields(cfg):
    """A Float8LinearConfig (the reference's or this project's) as plain data: enums by value, dtypes by name."""
    def plain(v):
        if dataclasses.is_dataclass(v):
            return {f.name: plain(getattr(v, f.name)) for f in dataclasses.fields(v)}
        if isinstance(v, enum.Enum):
            return v.value
        if isinstance(v, torch.dtype):
            return str(v)
        return v
    return plain(cfg)


def edge_tensor():
    g = torch.Generator().manual_seed(1)
    e = torch.randn(80, 48, generator=g)
    e[3, :] = 0.0
    e[:, 5] = 0.0
    e[7, 11] = torch.finfo(torch.bfloat16).max
    e[20, 9] = 1e-20
    return e.to(torch.bfloat16)


def sqnr(x, ref):
    return (10 * torch.log10(ref.double().pow(2).sum() / (x.double() - ref.double()).pow(2).sum())).item()


def main():
    from torchao.float8.config import CastConfig, Float8LinearConfig, ScalingGranularity, e4m3_dtype
    from torchao.float8.float8_linear import Float8Linear
    from torchao.float8.float8_scaling_utils import hp_tensor_to_float8_dynamic
    from torchao.float8.float8_training_tensor import LinearMMConfig

    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    go = (torch.randn(B, T, N, generator=g) * 0.01).to(torch.bfloat16)
    edge = edge_tensor()
    out = {"x": bits(x), "w": bits(w), "go": bits(go), "edge": bits(edge)}

    for name, t in (("x", x.reshape(-1, K)), ("go", go.reshape(-1, N)), ("w", w), ("edge", edge)):
        for tag, dim in AXES:
            gran = ScalingGranularity.TENSORWISE if dim is None else ScalingGranularity.AXISWISE
            scales = []
            for pow2 in (False, True):
                f8 = hp_tensor_to_float8_dynamic(t, e4m3_dtype, LinearMMConfig(), scaling_granularity=gran, axiswise_dim=dim,
                                                 round_scales_to_power_of_2=pow2)
                q, s = f8._data.view(torch.uint8).numpy().copy(), f8._scale.to(torch.float32).numpy().copy()
                assert q.shape == tuple(t.shape) and not np.any((q & 0x7F) == 0x7F), "a non-finite code"
                key = "%s_%s%d" % (name, tag, pow2)
                out[key + "_q"], out[key + "_s"] = q, s
                scales.append(s)
            cleared = (scales[0].view(np.uint32) & np.uint32(0xFF800000)).view(np.float32)
            assert np.array_equal(scales[1].view(np.uint32), cleared.view(np.uint32)), "exp2(floor(log2(s))) is not s with its mantissa cleared"

    x2, go2 = x.reshape(-1, K).float(), go.reshape(-1, N).float()
    y32, gi32, gw32 = x2 @ w.float().t(), go2 @ w.float(), go2.t() @ x2
    configs = {
        "rowwise": Float8LinearConfig.from_recipe_name("rowwise"),
        "rowwise_with_gw_hp": Float8LinearConfig.from_recipe_name("rowwise_with_gw_hp"),
        "tensorwise_e4m3": Float8LinearConfig(cast_config_grad_output=CastConfig(target_dtype=e4m3_dtype)),
    }
    for tag in RUNS:
        lin = torch.nn.Linear(K, N, bias=False).to(torch.bfloat16)
        lin.weight.data.copy_(w)
        m = Float8Linear.from_float(lin, dataclasses.replace(configs[tag], emulate=True))
        x_ = x.clone().requires_grad_(True)
        y = m(x_)
        y.backward(go)
        assert y.dtype == x_.grad.dtype == m.weight.grad.dtype == torch.bfloat16
        print("%-19s SQNR vs fp32: out %.2f dB, grad_input %.2f dB, grad_weight %.2f dB" % (
            tag, sqnr(y.reshape(-1, N), y32), sqnr(x_.grad.reshape(-1, K), gi32), sqnr(m.weight.grad, gw32)))
        out["out_" + tag], out["gi_" + tag], out["gw_" + tag] = bits(y), bits(x_.grad), bits(m.weight.grad)

    out["recipes"] = np.array(json.dumps({n: config_fields(Float8LinearConfig.from_recipe_name(n)) for n in RECIPES}, sort_keys=True))

    # identical tensors once
    stored = {}
    for key in list(out):
        v = out[key]
        if key == "recipes" or v.dtype.kind == "U":
            continue
        same = next((k for k, u in stored.items() if u.shape == v.shape and u.dtype == v.dtype and np.array_equal(u, v)), None)
        if same is None:
            stored[key] = v
        else:
            out[key] = np.array(same)
            print("  %s has the bits of %s" % (key, same))
    np.savez_compressed(PATH, **out)
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
