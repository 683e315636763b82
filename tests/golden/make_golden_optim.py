"""Generate tests/golden/optim.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_optim.py

Everything runs on the CPU.  torchao/optim/adam.py single_param_adam is called EAGERLY (never through torch.compile) on the reference's own
state subclasses; the subclasses' copy_ and dequantize record the quantizers alone.  bf16 tensors are stored as uint16 bit patterns, fp8 codes
as bytes.  The file holds

  qmap_q8s / qmap_q8u / qmap_q4s / qmap_q4u   the reference's four tables (fp32)
  cases                                       a JSON list: name, family (q8 | q4 | fp8 | plain), adamw, bf16, amsgrad, betas, wd, lr, eps, shape,
                                              block_size, steps, quantized
  <c>_p0, <c>_g<t>, <c>_scalars<t>, <c>_dp<t> the parameter, step t's gradient (t = 1 ..), its eight scalars (optim_ref.SCALAR_NAMES), and p after it
                                              as the XOR of its bits with the bits before the step (a step moves few bits, so the file
                                              stays under 1 MiB); optim_ref.load_golden() puts <c>_p<t> back
  <c>_s<k>_codes<t> / _scale<t> / _data<t>    state k (0 exp_avg, 1 exp_avg_sq, 2 max_exp_avg_sq) after step t: codes and scale, or a plain moment
  quant_cases                                 a JSON list: name, kind (q8s | q8u | q4s | q4u | fp8), block_size
  <q>_x, <q>_codes, <q>_scale, <q>_deq        the planted input (fp32), what copy_ wrote, and dequantize() of that
  <q>_all_codes, <q>_all_scale, <q>_all_deq   every code (256 or 16) through dequantize under one scale

The maker asserts that tests/optim_ref.py reproduces every recorded byte, that ao_amd/optim/quant_utils.py builds the reference's tables bit
for bit, and tells the fused lerp from the unfused one: it prints, per case, on how many recorded values the unfused restatement differs.

Three things about the recording (the first two are stated in csrc/quant_math.h, "low-bit optimizer states"):
  sqrt       taken under CorrectlyRoundedSqrt below: ATen's CPU sqrt is MKL's and not correctly rounded; the maker prints what it would change
  amsgrad    on quantized states the reference's eager run raises for want of aten.maximum; the maker registers the dequantizing form
  gradients  carry 4 mantissa bits (bf16 with the low three cleared), so that the file compresses under 1 MiB; p0 keeps every bit, and
             every intermediate of the step is a full fp32 value
"""
import contextlib
import json
import math
import os
import sys

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import optim_ref as R  # noqa: E402

from ao_amd.optim.adam import step_scalars  # noqa: E402
from ao_amd.optim.quant_utils import qmap_values  # noqa: E402
from torchao.optim import subclass_4bit as ref4  # noqa: E402
from torchao.optim import subclass_8bit as ref8  # noqa: E402
from torchao.optim import subclass_fp8 as reffp8  # noqa: E402
from torchao.optim.adam import single_param_adam  # noqa: E402


# amsgrad on a QUANTIZED state: single_param_adam calls torch.maximum(max_exp_avg_sq.float(), v), and the reference's subclasses implement no
# aten.maximum -- its eager run raises NotImplementedError there.  The maker registers, through the reference's own `implements`, the one
# form its lerp already has (dequantize the subclass argument, then the plain op): the contract's vmax = max(dequantized vmax_old, v).
# Plain states need nothing of the kind.
for _cls in (ref8.OptimState8bit, ref4.OptimState4bit, reffp8.OptimStateFp8):
    def _maximum(func, types, args, kwargs, _cls=_cls):
        return func(*[a.dequantize() if isinstance(a, _cls) else a for a in args], **kwargs)
    _cls.implements(torch.ops.aten.maximum.default)(_maximum)


def bits(t):
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy().reshape(-1)
    if t.dtype == torch.float8_e4m3fn:
        return t.contiguous().view(torch.uint8).numpy().copy().reshape(-1)
    return t.contiguous().numpy().copy().reshape(-1)


def ref_qmaps():
    return {
        "q8s": np.array(ref8.get_qmap_signed(), dtype=np.float32), "q8u": np.array(ref8.get_qmap_unsigned(), dtype=np.float32),
        "q4s": np.array(ref4.get_qmap_signed(), dtype=np.float32), "q4u": np.array(ref4.get_qmap_unsigned(), dtype=np.float32),
    }


def ref_zeros(family, p, signed, block_size):
    if family == "q8":
        return ref8.OptimState8bit.zeros(p.shape, signed, block_size, "cpu", dtype=p.dtype)
    if family == "q4":
        return ref4.OptimState4bit.zeros(p.shape, signed, block_size, "cpu", dtype=p.dtype)
    if family == "fp8":
        return reffp8.OptimStateFp8.zeros(p.shape, block_size, "cpu", dtype=p.dtype)
    raise AssertionError(family)


def state_fields(s):
    if type(s) is torch.Tensor:
        return {"data": bits(s)}
    return {"codes": bits(s.codes), "scale": bits(s.scale)}


CASES = []


def case(name, family, adamw, bf16, shape, block_size, amsgrad=False, betas=(0.9, 0.999), wd=None, lr=1e-3, steps=2, grad_scale=0.02):
    CASES.append(dict(name=name, family=family, adamw=adamw, bf16=bf16, amsgrad=amsgrad, betas=list(betas), wd=(1e-2 if adamw else 0.0) if wd is None
                      else wd, lr=lr, eps=1e-8, shape=list(shape), block_size=block_size, steps=steps, grad_scale=grad_scale))


EXACT = (0.75, 0.9375)
# A covering set, not the full product (the file stays under 1 MiB, and a quantized case cannot have fewer than 4096 elements): every format
# meets AdamW and Adam, bf16 and fp32 (the fp32 case alternates AdamW / Adam over the formats), amsgrad on and off, both beta pairs, both
# weight decays, and the five shapes.
for i, (fam, bs) in enumerate((("q8", 256), ("q4", 128), ("fp8", 256))):
    case(f"{fam}_adamw_bf16", fam, True, True, (4096,), bs)
    case(f"{fam}_straddle", fam, True, True, (48, 96), bs, betas=EXACT, wd=0.0, lr=3e-3)                  # 4608 elements: blocks straddle rows
    case(f"{fam}_plus_block", fam, False, True, (4096 + bs,), bs, amsgrad=True, wd=1e-2)
    case(f"{fam}_b2048_f32", fam, i % 2 == 1, False, (4096,), 2048, amsgrad=True, wd=1e-2)               # (AdamW for q4, Adam for q8 and fp8)
    case(f"{fam}_b64", fam, False, True, (4096,), 64, betas=EXACT, wd=0.0)
# plain states: too small, indivisible, and _AdamW
case("plain_1", "q8", True, True, (1,), 256)
case("plain_7", "q4", False, False, (7,), 128, wd=1e-2, amsgrad=True)
case("plain_4095", "fp8", False, True, (4095,), 256, wd=1e-2)
case("plain_4097", "q8", True, True, (4097,), 256)
case("plain_adamw_4096", "plain", True, True, (4096,), 0)
case("plain_adamw_64_f32", "plain", True, False, (64,), 0, amsgrad=True, betas=EXACT)
case("plain_subnormal_f32", "plain", True, False, (70,), 0, grad_scale=1e-20, wd=0.0, steps=3)   # g g and v are fp32 subnormals


class CorrectlyRoundedSqrt(TorchDispatchMode):
    """aten.sqrt of an fp32 tensor through float64 (exact for fp32: a float64 root rounded to fp32 is the correctly rounded fp32 root).
    ATen's CPU sqrt of a contiguous tensor is MKL's vsSqrt, accurate to under an ulp but NOT correctly rounded (about 0.6% of random
    inputs are an ulp off), and which inputs depends on the MKL build and the processor: bytes no kernel can be asked to reproduce.  The
    contract's sqrt is the IEEE one, so the recording is taken under this mode; main() prints how many recorded values MKL's root changes."""

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func is torch.ops.aten.sqrt.default and args[0].dtype == torch.float32:
            return args[0].double().sqrt().float()
        return func(*args, **(kwargs or {}))


def reference_run(c, correct_sqrt=True):
    """single_param_adam, eagerly, for c["steps"] steps -> the recorded arrays of the case (without its name)"""
    g = torch.Generator().manual_seed(1000 + len(c["name"]) * 7 + sum(c["shape"]))
    dtype = torch.bfloat16 if c["bf16"] else torch.float32
    n = math.prod(c["shape"])
    p = (torch.randn(c["shape"], generator=g) * 0.1).to(dtype)
    quantized = c["family"] != "plain" and n >= 4096 and n % c["block_size"] == 0
    c["quantized"] = quantized
    make = (lambda signed: ref_zeros(c["family"], p, signed, c["block_size"])) if quantized else (lambda signed: torch.zeros_like(p))
    states = [make(True), make(False)] + ([make(False)] if c["amsgrad"] else [])
    rec = {"p0": bits(p)}
    lr, step = torch.tensor(c["lr"], dtype=torch.float32), torch.tensor(0.0)
    for t in range(1, c["steps"] + 1):
        row = torch.exp(torch.randn(c["shape"][0], *([1] * (len(c["shape"]) - 1)), generator=g) * 0.5) if len(c["shape"]) > 1 else 1.0
        grad = (torch.randn(c["shape"], generator=g) * c["grad_scale"] * row).to(torch.bfloat16)
        grad = (grad.view(torch.int16) & -8).view(torch.bfloat16).to(dtype)   # 4 mantissa bits: the file compresses; p0 keeps every bit
        step += 1
        with (CorrectlyRoundedSqrt() if correct_sqrt else contextlib.nullcontext()):
            single_param_adam(p, grad, step, states[0], states[1], states[2] if c["amsgrad"] else None, lr, c["betas"][0], c["betas"][1], c["wd"],
                              c["eps"], c["adamw"], False)
        rec[f"g{t}"], rec[f"p{t}"] = bits(grad), bits(p)
        rec[f"scalars{t}"] = np.array(step_scalars(lr, c["betas"][0], c["betas"][1], c["wd"], c["eps"], step), dtype=np.float32)
        for k, s in enumerate(states):
            for field, v in state_fields(s).items():
                rec[f"s{k}_{field}{t}"] = v
    return rec


def restate(c, rec, qmaps, lerp_fn):
    """the restatement over the recorded inputs -> how many recorded values it misses"""
    n = math.prod(c["shape"])
    states = R.new_states(c["family"] if c["quantized"] else "plain", n, c["block_size"], qmaps, c["bf16"], c["amsgrad"])
    p, missed = rec["p0"], 0
    for t in range(1, c["steps"] + 1):
        p = R.adam_step(p, rec[f"g{t}"], states, dict(zip(R.SCALAR_NAMES, rec[f"scalars{t}"])), c["adamw"], c["bf16"], lerp_fn=lerp_fn)
        assert p.dtype == rec[f"p{t}"].dtype
        missed += int((p != rec[f"p{t}"]).sum())
        for k, s in enumerate(states):
            for field, v in s.fields().items():
                assert v.dtype == rec[f"s{k}_{field}{t}"].dtype
                missed += int((v != rec[f"s{k}_{field}{t}"]).sum())
    return missed


def run_case(out, c, qmaps):
    rec = reference_run(c)
    raw = reference_run(c, correct_sqrt=False)
    mkl_diff = sum(int((rec[k] != raw[k]).sum()) for k in rec)
    missed = restate(c, rec, qmaps, R.lerp)
    assert missed == 0, (c["name"], "the restatement misses", missed, "recorded values")
    unfused_diff = restate(c, rec, qmaps, R.lerp_unfused)
    for k, v in R.pack_steps(rec, c["steps"]).items():
        out[f"{c['name']}_{k}"] = v
    print(f"{c['name']:28s} n={math.prod(c['shape']):5d} quantized={c['quantized']!s:5s} restatement: equal;  unfused lerp misses {unfused_diff:4d} "
          f"recorded values;  MKL's sqrt changes {mkl_diff}")
    return unfused_diff, mkl_diff


def planted(kind, qmap, bs):
    """fp32 [blocks x bs]: what the quantizers can get wrong"""
    g = torch.Generator().manual_seed(len(kind) * 31 + bs)
    signed = kind in ("q8s", "q4s", "fp8")
    grid = torch.tensor(qmap) if qmap is not None else torch.tensor(R.E4M3_POS, dtype=torch.float32) / 448.0
    if kind == "fp8":
        grid = torch.cat([-grid.flip(0), grid])
    mids = (grid[:-1] + grid[1:]) / 2.0
    rows = []

    def block(vals, fill=0.0):
        b = torch.full((bs,), float(fill))
        b[: len(vals)] = torch.as_tensor(vals, dtype=torch.float32)
        rows.append(b)

    block([])                                              # all zero
    block([], fill=0.37109375)                             # one repeated value
    for scale in (1.0, 0.0123):                            # table entries and midpoints under an exact and an inexact scale
        for vals in (grid, mids):
            for i in range(0, len(vals), bs - 1):
                block(torch.cat([vals[i:i + bs - 1] * scale, torch.tensor([scale])]))  # (the last element pins the amax)
    block([3.5, -3.5 if signed else 3.5, 1.75, 0.0])      # -1.0 and +1.0 of scale
    tiny = torch.randn(bs, generator=g) * 1e-13            # amax below 1e-12
    block(tiny if signed else tiny.abs())
    r = torch.randn(bs, generator=g)
    block(r if signed else r.abs())
    return torch.stack(rows).reshape(-1)


def run_quant(out, kind, bs, qmaps):
    qmap = qmaps.get(kind)
    x = planted(kind, qmap, bs)
    if kind == "fp8":
        s = reffp8.OptimStateFp8.zeros(x.shape, bs, "cpu")
        all_codes = torch.arange(256, dtype=torch.uint8)
        all_codes[(all_codes & 0x7F) == 0x7F] = 0          # (the two NaN codes are outside the contract)
        every = reffp8.OptimStateFp8(all_codes.view(torch.float8_e4m3fn), torch.tensor([0.7]))
    elif kind in ("q8s", "q8u"):
        s = ref8.OptimState8bit.zeros(x.shape, kind == "q8s", bs, "cpu")
        every = ref8.OptimState8bit(torch.arange(256, dtype=torch.uint8), torch.tensor([0.7]), s.qmap, kind == "q8s")
    else:
        s = ref4.OptimState4bit.zeros(x.shape, kind == "q4s", bs, "cpu")
        codes = torch.arange(16, dtype=torch.uint8).repeat(bs // 16)
        every = ref4.OptimState4bit((codes[::2] << 4) | codes[1::2], torch.tensor([0.7]), s.qmap, kind == "q4s", (bs,))
    s.copy_(x)
    name = f"quant_{kind}"
    out[f"{name}_x"], out[f"{name}_codes"], out[f"{name}_scale"], out[f"{name}_deq"] = bits(x), bits(s.codes), bits(s.scale), bits(s.dequantize())
    out[f"{name}_all_codes"], out[f"{name}_all_scale"], out[f"{name}_all_deq"] = bits(every.codes), bits(every.scale), bits(every.dequantize())
    codes, scale = R.quantize(kind, out[f"{name}_x"], bs, qmap)
    assert np.array_equal(codes, out[f"{name}_codes"]), (name, int((codes != out[f"{name}_codes"]).sum()))
    assert np.array_equal(scale, out[f"{name}_scale"]), name
    assert np.array_equal(R.dequantize(kind, codes, scale, bs, qmap).view(np.uint32), out[f"{name}_deq"].view(np.uint32)), name
    every_bs = every.codes.numel() * (2 if kind in ("q4s", "q4u") else 1)
    assert np.array_equal(R.dequantize(kind, out[f"{name}_all_codes"], out[f"{name}_all_scale"], every_bs, qmap).view(np.uint32),
                          out[f"{name}_all_deq"].view(np.uint32)), name
    used = len(set((R.unpack4(codes) if kind in ("q4s", "q4u") else codes).tolist()))
    print(f"{name:28s} n={x.numel():5d} block={bs} codes used: {used}")
    return dict(name=name, kind=kind, block_size=bs, all_block_size=every_bs)


def main():
    out = {}
    qmaps = ref_qmaps()
    for k, v in qmaps.items():
        out[f"qmap_{k}"] = v
        mine = np.array(qmap_values(int(k[1]), k[2] == "s"), dtype=np.float32)
        assert np.array_equal(mine.view(np.uint32), v.view(np.uint32)), f"ao_amd/optim/quant_utils.py builds another {k} table"
    results = {c["name"]: run_case(out, c, qmaps) for c in CASES}
    diffs = {k: v[0] for k, v in results.items()}
    print("MKL's sqrt changes", sum(v[1] for v in results.values()), "recorded values in", sum(v[1] > 0 for v in results.values()), "of", len(CASES), "cases")
    exact = [n for n, c in ((c["name"], c) for c in CASES) if c["betas"] == list(EXACT)]
    assert all(diffs[n] == 0 for n in exact), "betas (0.75, 0.9375): the fused and the unfused lerp must agree"
    default = [c["name"] for c in CASES if c["betas"] != list(EXACT) and math.prod(c["shape"]) >= 4096]
    print("unfused lerp differs somewhere in", sum(diffs[n] > 0 for n in default), "of", len(default), "default-beta cases of >= 4096 elements")
    out["cases"] = np.array(json.dumps(CASES))
    out["quant_cases"] = np.array(json.dumps([run_quant(out, k, 128 if k.startswith("q4") else 256, qmaps) for k in ("q8s", "q8u", "q4s", "q4u", "fp8")]))
    path = os.path.join(HERE, "optim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
