"""Generate tests/golden/qat.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_qat.py

Everything runs on the CPU.  bf16 tensors are stored as uint16 bit patterns.  The archive is a zip with LZMA members (numpy.load reads
it like any .npz): the long-row float8 cases repeat their rows, which LZMA folds and deflate's 32 KiB window does not.

  int4_cases            [[g, N, K], ...]: g in {32, 64, 128, 256} at (N, K) in {(1, g), (3, 3g), (17, 5g)}
  int4_g{g}_{N}x{K}_w   the weight; _out Int4WeightFakeQuantizer's forward; _go a gradient; _gw the reference's OWN autograd gradient
                        planted: group (0, 0) holds a tie for the maximum (columns TIE_MAX) and for the minimum (TIE_MIN) and a -0.0;
                        where there are more groups: an all-equal non-zero group, an all-zero group with a -0.0, a group of +-2^-20 ..
                        2^6, an all-(+0) group
  fp8_names             the float8 cases: r{R}c{C} for C in {16, 48, 512, 1040, 8208} at R in {1, 3, 67}, r2c16400 (a row longer than the
                        registers hold), b2x5x48_{0,1,2} (one [2, 5, 48] input under the three bound settings)
  fp8_{name}_x          the input; _out Float8FakeQuantizer's forward (PerRow, e4m3); _cfg [hp_value_lb, hp_value_ub] (NaN = None).  The
                        reference's gradient is NOT recorded: it rounds the incoming gradient to e4m3.
                        planted: row 0 a +- tie for max|x|; from 3 rows: row 1 below lb = 1e-12, row 2 above ub = 3; from 67 rows: row 5
                        all zero with a -0.0 (NaN in the reference where there is no lower bound: recorded as it comes), row 6 tiny.
                        The 67-row cases from C = 512 repeat five rows in turn after their first twelve, one marker element apart
                        (every row still differs from every other): the archive stays under 1 MiB, the grid stays whole.
  sqnr_int4 [4]         for g = 32 .. 256 on a 64 x 512 N(0, 0.02^2) weight: Int4Tensor's dequantisation bf16(bf16(q bf16(s)) + bf16(z))
                        against the fake-quantized weight, in dB
  sqnr_fp8              a [32, 256] x [128, 256] linear through exact e4m3 x e4m3 products and the two scales against F.linear of the
                        fake-quantized operands, in dB
The maker asserts what tests/test_qat_host.py asserts again: the restatement (tests/qat_ref.py) gives the reference's forward bytes, the
reference's int4 gradient lies inside the bound of the float64 formula, and at the planted ties the formula leaves the bound around G.
"""
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

GROUPS = (32, 64, 128, 256)
FP8_COLS = (16, 48, 512, 1040, 8208)
FP8_ROWS = (1, 3, 67)
BOUNDS = ((None, None), (1e-12, None), (1e-12, 3.0))
TIE_MAX, TIE_MIN, NEG_ZERO = (1, -2), (3, -5), 5  # columns inside group (0, 0) / row 0


def bf(t):
    return t.to(torch.bfloat16)


def int4_weight(gen, g, n, k):
    std = torch.where(torch.arange(n) % 2 == 0, 1.0, 0.02).reshape(n, 1)
    w = bf(torch.randn(n, k, generator=gen) * std).view(n, k // g, g).clone()
    top = bf(w[0, 0].float().abs().max() * 1.25)
    for c in TIE_MAX:
        w[0, 0, c] = top
    for c in TIE_MIN:
        w[0, 0, c] = -bf(top.float() * 1.125)
    w[0, 0, NEG_ZERO] = -0.0
    if k // g >= 3 and n >= 2:
        w[0, 1] = 0.375
        w[0, 2] = 0.0
        w[0, 2, 7] = -0.0
        e = torch.arange(g) % 27 - 20
        w[1, 0] = bf(torch.exp2(e.float()) * torch.where(torch.arange(g) % 3 == 0, -1.0, 1.0))
        w[1, 1] = 0.0
    return w.view(n, k).contiguous()


def fp8_input(gen, r, c):
    distinct = min(r, 12) if r * c > 30000 else r  # the planted rows 0 .. 6, then five rows in turn
    scale = torch.tensor([1.0, 0.02, 8.0, 2.0 ** -10, 1.0])[torch.arange(distinct) % 5].reshape(distinct, 1)
    x = bf(torch.randn(distinct, c, generator=gen) * scale)
    if distinct < r:
        idx = torch.arange(r)
        idx[distinct:] = 7 + idx[distinct:] % 5
        x = x[idx].clone()
        for i in range(distinct, r):
            x[i, (8 * i + 1) % c] = i / 128.0  # rows stay distinct
    top = bf(x[0].float().abs().max() * 1.5)
    x[0, 2], x[0, c - 3] = top, -top
    if r >= 3:
        x[1] = bf(x[1].float() * (1e-14 / max(float(x[1].float().abs().max()), 1e-30)))
        x[2] = bf(x[2].float() * (12.0 / float(x[2].float().abs().max())))
    if r >= 67:
        x[5] = 0.0
        x[5, 4] = -0.0
        x[6] = bf(x[6].float() * 1e-16)
    return x.contiguous()


def main():
    from torchao.quantization.qat.fake_quantize_config import Float8FakeQuantizeConfig, Int4WeightFakeQuantizeConfig
    from torchao.quantization.qat.fake_quantizer import Float8FakeQuantizer, Int4WeightFakeQuantizer

    import qat_ref as R

    gen = torch.Generator().manual_seed(0)
    out = {"tie_max": np.array(TIE_MAX), "tie_min": np.array(TIE_MIN)}
    cases, worst = [], 0.0
    for g in GROUPS:
        for n, k in ((1, g), (3, 3 * g), (17, 5 * g)):
            w = int4_weight(gen, g, n, k)
            go = bf(torch.randn(n, k, generator=gen) * (1e-3 if n != 3 else 1.0))
            wr = w.clone().requires_grad_()
            y = Int4WeightFakeQuantizer(Int4WeightFakeQuantizeConfig(group_size=g, activation_dtype=torch.bfloat16))(wr)
            y.backward(go)
            assert y.dtype == torch.bfloat16 and wr.grad.dtype == torch.bfloat16
            assert np.array_equal(R.bits(y.detach()), R.bits(R.int4_fake_quantize(w, g))), (g, n, k)
            want, mag = R.int4_fake_quantize_bwd(w, go, g)
            err = (wr.grad.double() - want).abs() / R.bound(want, mag)
            worst = max(worst, float(err.max()))
            assert float(err.max()) <= 1.0, (g, n, k, float(err.max()))
            for c in TIE_MAX + TIE_MIN:  # the range term is visible: without it the bound around G would not hold there
                c = c % g
                assert abs(float(want[0, c]) - float(go[0, c])) > float(R.bound(want, mag)[0, c]), (g, n, k, c)
            name = f"int4_g{g}_{n}x{k}"
            out[f"{name}_w"], out[f"{name}_out"], out[f"{name}_go"], out[f"{name}_gw"] = R.bits(w), R.bits(y.detach()), R.bits(go), R.bits(wr.grad)
            cases.append([g, n, k])
    out["int4_cases"] = np.array(cases, dtype=np.int64)
    print("int4: the reference's gradient against the float64 formula, worst error / bound:", worst)

    names = []

    def record_fp8(name, x, lb, ub):
        y = Float8FakeQuantizer(Float8FakeQuantizeConfig(hp_value_lb=lb, hp_value_ub=ub))(x)
        assert y.dtype == torch.bfloat16 and y.shape == x.shape
        assert np.array_equal(R.bits(y), R.bits(R.fp8_fake_quantize(x, lb, ub))), name
        out[f"fp8_{name}_x"], out[f"fp8_{name}_out"] = R.bits(x), R.bits(y)
        out[f"fp8_{name}_cfg"] = np.array([np.nan if v is None else v for v in (lb, ub)], dtype=np.float64)
        names.append(name)

    for ci, c in enumerate(FP8_COLS):
        for ri, r in enumerate(FP8_ROWS):
            record_fp8(f"r{r}c{c}", fp8_input(gen, r, c), *BOUNDS[(ci + ri) % 3])  # every row count meets every bound setting
    record_fp8("r2c16400", fp8_input(gen, 2, 16400), 1e-12, None)
    x3 = fp8_input(gen, 10, 48).reshape(2, 5, 48)
    for j, (lb, ub) in enumerate(BOUNDS):
        record_fp8(f"b2x5x48_{j}", x3, lb, ub)
    out["fp8_names"] = np.array(names)

    w = bf(torch.randn(64, 512, generator=gen) * 0.02)
    sq = []
    for g in GROUPS:
        q, s, z = R.int4_codes(w, g)
        deq = bf(bf(q * bf(s).float()).float() + bf(z).float()).reshape(w.shape)
        sq.append(R.sqnr_db(deq, R.int4_fake_quantize(w, g)))
    out["sqnr_int4"] = np.array(sq, dtype=np.float64)
    x, wt = bf(torch.randn(32, 256, generator=gen)), bf(torch.randn(128, 256, generator=gen) * 0.02)
    (qx, sx), (qw, sw) = R.fp8_codes(x), R.fp8_codes(wt)
    exact = bf(((qx.double() @ qw.double().t()) * sx.double() * sw.double().t()).float())
    fake = torch.nn.functional.linear(R.fp8_fake_quantize(x), R.fp8_fake_quantize(wt))
    out["sqnr_fp8"] = np.array(R.sqnr_db(exact, fake), dtype=np.float64)

    path = os.path.join(HERE, "qat.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as zf:
        for key, value in out.items():
            with zf.open(key + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(value), allow_pickle=False)
    print(os.path.getsize(path), "bytes;", "sqnr_int4", out["sqnr_int4"], "sqnr_fp8", out["sqnr_fp8"])


if __name__ == "__main__":
    main()
