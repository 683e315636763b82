"""Quantization-aware training on the GPU: the four kernels of ao_amd/csrc/qat_kernels.hip against the reference's recorded bytes
(tests/golden/qat.npz) and the CPU restatement (tests/qat_ref.py), FakeQuantizedLinear against F.linear autograd on the restatement's
operands, and quantize_ prepare -> one optimizer step -> convert for both base configs.

Forward: byte for byte.  Backward: inside |ref| 2^-8 + mag 2^-16 of the float64 formula, mag = sum |G| over the group (int4) or the row
(fp8) -- qat_ref.bound.  Every launch runs twice and gives the same bytes."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qat_ref as R  # noqa: E402
from ao_amd import ops  # noqa: E402
from ao_amd.quantization import (  # noqa: E402
    Float8DynamicActivationFloat8WeightConfig,
    Float8Tensor,
    Int4Tensor,
    Int4WeightOnlyConfig,
    PerRow,
    quantize_,
)
from ao_amd.quantization.qat import (  # noqa: E402
    FakeQuantizedLinear,
    Float8FakeQuantizeConfig,
    Int4WeightFakeQuantizeConfig,
    QATConfig,
)

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qat.npz"))
INT4_CASES = [tuple(int(v) for v in c) for c in GOLD["int4_cases"]]
FP8_NAMES = [str(n) for n in GOLD["fp8_names"]]
# seeded Gaussian inputs: the fixture's shapes, and the row lengths at which the fp8 launch takes another register depth (2, 4 and 8
# vectors a thread; past 16384 elements the row is walked twice)
FP8_GAUSS = [(r, c) for c in (16, 48, 512, 1040, 8208) for r in (1, 3, 67)] + [(3, 4096), (3, 6144), (2, 16384), (2, 16400)]
BOUNDS = ((None, None), (1e-12, None), (1e-12, 3.0))


def same_bits(a, b):
    return np.array_equal(R.bits(a.cpu()) if isinstance(a, torch.Tensor) else a, R.bits(b.cpu()) if isinstance(b, torch.Tensor) else b)


def twice(fn, *args):
    a, b = fn(*args), fn(*args)
    torch.cuda.synchronize()
    assert same_bits(a, b), "two launches on the same input gave different bytes"
    return a


def assert_inside_bound(got, want, mag):
    got = got.cpu().double()
    assert bool((got.isnan() == want.isnan()).all())
    ok = ~want.isnan()
    err = (got - want).abs()[ok] / R.bound(want, mag)[ok]
    assert err.numel() == 0 or float(err.max()) <= 1.0, f"worst error / bound = {float(err.max())}"


def gaussian(seed, shape, std):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=gen) * std).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def int4_fixture(g, n, k):
    name = f"int4_g{g}_{n}x{k}"
    w, go = R.from_bits(GOLD[f"{name}_w"]), R.from_bits(GOLD[f"{name}_go"])
    return w, go, R.int4_fake_quantize(w, g), R.int4_fake_quantize_bwd(w, go, g)


@functools.lru_cache(maxsize=None)
def fp8_fixture(name):
    lb, ub = (None if math.isnan(v) else float(v) for v in GOLD[f"fp8_{name}_cfg"])
    x = R.from_bits(GOLD[f"fp8_{name}_x"])
    go = gaussian(5, x.shape, 1e-3)
    return x, go, lb, ub, R.fp8_fake_quantize(x, lb, ub), R.fp8_fake_quantize_bwd(x, go, lb, ub)


# ---- the kernels over the fixture -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,n,k", INT4_CASES)
def test_int4_kernels_on_the_fixture(g, n, k):
    w, go, out_ref, (grad_ref, mag) = int4_fixture(g, n, k)
    out = twice(ops.qat_int4_fake_quantize, w.cuda(), g)
    assert same_bits(out, GOLD[f"int4_g{g}_{n}x{k}_out"]) and same_bits(out, out_ref)
    grad = twice(ops.qat_int4_fake_quantize_bwd, w.cuda(), go.cuda(), g)
    assert grad.dtype == torch.bfloat16 and grad.shape == w.shape
    assert_inside_bound(grad, grad_ref, mag)


@pytest.mark.parametrize("name", FP8_NAMES)
def test_fp8_kernels_on_the_fixture(name):
    x, go, lb, ub, out_ref, (grad_ref, mag) = fp8_fixture(name)
    out = twice(ops.qat_fp8_fake_quantize_rowwise, x.cuda(), lb, ub)
    assert out.shape == x.shape
    assert same_bits(out, GOLD[f"fp8_{name}_out"]) and same_bits(out, out_ref)
    grad = twice(ops.qat_fp8_fake_quantize_rowwise_bwd, x.cuda(), go.cuda(), lb, ub)
    assert grad.dtype == torch.bfloat16 and grad.shape == x.shape
    assert_inside_bound(grad, grad_ref, mag)


# ---- seeded Gaussian inputs against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("std", [1.0, 0.02])
@pytest.mark.parametrize("g,n,k", INT4_CASES)
def test_int4_kernels_on_gaussian_inputs(g, n, k, std):
    w, go = gaussian(g + n, (n, k), std), gaussian(g + n + 1, (n, k), 1e-3)
    assert same_bits(twice(ops.qat_int4_fake_quantize, w.cuda(), g), R.int4_fake_quantize(w, g))
    assert_inside_bound(twice(ops.qat_int4_fake_quantize_bwd, w.cuda(), go.cuda(), g), *R.int4_fake_quantize_bwd(w, go, g))


@pytest.mark.parametrize("r,c", FP8_GAUSS)
def test_fp8_kernels_on_gaussian_inputs(r, c):
    std = 1.0 if (r + c // 16) % 2 else 0.02
    lb, ub = BOUNDS[(r + c // 16) % 3]
    x, go = gaussian(r + c, (r, c), std), gaussian(r + c + 1, (r, c), 1e-3)
    assert same_bits(twice(ops.qat_fp8_fake_quantize_rowwise, x.cuda(), lb, ub), R.fp8_fake_quantize(x, lb, ub))
    assert_inside_bound(twice(ops.qat_fp8_fake_quantize_rowwise_bwd, x.cuda(), go.cuda(), lb, ub), *R.fp8_fake_quantize_bwd(x, go, lb, ub))


def test_empty_and_strided_inputs():
    w = gaussian(1, (4, 64), 1.0).cuda()
    assert ops.qat_int4_fake_quantize(w[:0], 32).shape == (0, 64) and ops.qat_fp8_fake_quantize_rowwise(w[:0]).shape == (0, 64)
    assert ops.qat_int4_fake_quantize_bwd(w[:0], w[:0], 32).shape == (0, 64)
    wide = gaussian(2, (4, 128), 1.0).cuda()
    assert same_bits(ops.qat_int4_fake_quantize(wide[:, :64], 32), R.int4_fake_quantize(wide[:, :64].cpu(), 32))  # a strided view is copied
    assert same_bits(ops.qat_fp8_fake_quantize_rowwise(wide[:, 64:]), R.fp8_fake_quantize(wide[:, 64:].cpu()))


# ---- FakeQuantizedLinear ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ["int4", "fp8"])
def test_fake_quantized_linear_against_autograd_on_the_restatements_operands(pair):
    m, k, n = 5, 96, 48
    x, w, bias, go = gaussian(1, (m, k), 1.0), gaussian(2, (n, k), 0.02), gaussian(3, (n,), 0.1), gaussian(4, (m, n), 1e-2)
    if pair == "int4":
        act, wc = None, Int4WeightFakeQuantizeConfig(group_size=32)
        xq, wq = x, R.int4_fake_quantize(w, 32)
    else:
        act, wc = Float8FakeQuantizeConfig(hp_value_lb=1e-12), Float8FakeQuantizeConfig()
        xq, wq = R.fp8_fake_quantize(x, 1e-12), R.fp8_fake_quantize(w)
    lin = FakeQuantizedLinear(k, n, True, activation_config=act, weight_config=wc, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(bias)
    xg = x.cuda().requires_grad_()
    y = lin(xg)
    y.backward(go.cuda())
    xe, we, be = (t.cuda().requires_grad_() for t in (xq, wq, bias))
    ye = F.linear(xe, we, be)
    ye.backward(go.cuda())
    assert same_bits(y.detach(), ye.detach()) and same_bits(lin.bias.grad, be.grad)
    if pair == "int4":
        assert same_bits(xg.grad, xe.grad)  # no activation quantizer: the matmul's own gradient
        assert_inside_bound(lin.weight.grad, *R.int4_fake_quantize_bwd(w, we.grad.cpu(), 32))
    else:  # the matmul's gradients, then each fake quantizer's backward
        assert_inside_bound(xg.grad, *R.fp8_fake_quantize_bwd(x, xe.grad.cpu(), 1e-12))
        assert_inside_bound(lin.weight.grad, *R.fp8_fake_quantize_bwd(w, we.grad.cpu()))
    lin.weight_fake_quantizer.enabled = False
    if lin.activation_fake_quantizer is not None:
        lin.activation_fake_quantizer.enabled = False
    assert same_bits(lin(x.cuda()).detach(), F.linear(x.cuda(), w.cuda(), bias.cuda()))


# ---- quantize_: prepare -> one optimizer step -> convert --------------------------------------------------------------------------------
def _train_one_step(model, x):
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    before = [p.detach().clone() for p in model.parameters()]
    model(x).float().pow(2).mean().backward()
    assert all(p.grad is not None and bool(p.grad.isfinite().all()) for p in model.parameters())
    opt.step()
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))


@pytest.mark.parametrize("gi,g", list(enumerate((32, 64, 128, 256))))
def test_quantize_prepare_train_convert_int4(gi, g):
    torch.manual_seed(g)
    model = nn.Sequential(nn.Linear(256, 256, bias=True), nn.Linear(256, 64, bias=False)).to(torch.bfloat16).cuda()
    base = Int4WeightOnlyConfig(group_size=g)
    quantize_(model, QATConfig(base, step="prepare"))
    assert all(type(mod) is FakeQuantizedLinear for mod in model)
    _train_one_step(model, torch.randn(8, 256, device="cuda", dtype=torch.bfloat16))
    trained = [mod.weight.detach().clone() for mod in model]
    quantize_(model, QATConfig(base, step="convert"))
    for mod, w in zip(model, trained):
        assert type(mod) is nn.Linear and type(mod.weight) is Int4Tensor
        fake = ops.qat_int4_fake_quantize(w, g)
        got = R.sqnr_db(mod.weight.dequantize().cpu(), fake.cpu())
        assert got >= float(GOLD["sqnr_int4"][gi]) - 3.0, (got, float(GOLD["sqnr_int4"][gi]))
    assert model(torch.randn(3, 256, device="cuda", dtype=torch.bfloat16)).shape == (3, 64)


def test_quantize_prepare_train_convert_float8():
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(256, 128, bias=False)).to(torch.bfloat16).cuda()
    base = Float8DynamicActivationFloat8WeightConfig(granularity=PerRow())
    quantize_(model, QATConfig(base, step="prepare"))
    assert type(model[0]) is FakeQuantizedLinear
    assert model[0].activation_fake_quantizer is not None and model[0].weight_fake_quantizer is not None
    _train_one_step(model, torch.randn(32, 256, device="cuda", dtype=torch.bfloat16))
    x = torch.randn(32, 256, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        prepared = model(x)
    quantize_(model, QATConfig(base, step="convert"))
    assert type(model[0]) is nn.Linear and type(model[0].weight) is Float8Tensor
    with torch.no_grad():
        got = R.sqnr_db(model(x).cpu(), prepared.cpu())
    assert got >= float(GOLD["sqnr_fp8"]) - 3.0, (got, float(GOLD["sqnr_fp8"]))
