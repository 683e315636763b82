"""torch restatement of the int8 / float8 weight-only linears (bf16 activation x 8-bit weight).
TEST INFRASTRUCTURE ONLY.  Paths relative to the reference torchao tree.  Pinned against tests/golden/wo8.npz, which
tests/golden/make_golden_wo8.py writes from the reference.

  int8   quantization/quantize_/workflows/int8/int8_tensor.py:346-359   m = mm(x, qdata.t().to(bf16)); y = m * scale.to(bf16); y += bias
  float8 quantization/quantize_/workflows/float8/float8_tensor.py:460-469 -> dequantize :255-275
         w = (qdata.to(f32) * scale).to(bf16); out = matmul(x, w.t()); out + bias

The sum over k is taken in float64 and rounded to fp32, then bf16 (the oracle's rounding, _parity.oracle_round); every later step is a
bf16 tensor op: fp32 arithmetic on bf16 values, rounded to nearest even.  Works on any device.
"""
import torch

FMT_INT8, FMT_E4M3 = 0, 1
FMTS = {"int8": FMT_INT8, "e4m3": FMT_E4M3}


def _bf16(v):
    return v.to(torch.float32).to(torch.bfloat16)


def weight(fmt, q, scale):
    """The bf16-valued matrix the sum multiplies, as float64 [N, K]: int8 codes as they are (the scale comes after the sum); e4m3 codes
    dequantized element by element, fp32 product rounded to bf16."""
    if fmt == FMT_INT8:
        return q.to(torch.float64)
    s = scale.reshape(-1, 1).to(torch.float32)
    return (q.to(torch.float32) * s).to(torch.bfloat16).to(torch.float64)


def sums(fmt, x, q, scale):
    """(m64, S): the float64 sum over k and the float64 sum of absolute products, [M, N]."""
    w = weight(fmt, q, scale)
    xd = x.to(torch.float64)
    return xd @ w.t(), xd.abs() @ w.abs().t()


def chain(fmt, m, scale, bias=None):
    """What follows the sum: m [M, N] float64 -> bf16 [M, N]."""
    t = _bf16(m)
    if fmt == FMT_INT8:
        s = scale.reshape(-1).to(torch.float32).to(torch.bfloat16)
        t = _bf16(t.to(torch.float32) * s.to(torch.float32))
    if bias is not None:
        t = _bf16(t.to(torch.float32) + bias.to(torch.bfloat16).to(torch.float32))
    return t


def linear(fmt, x, q, scale, bias=None):
    return chain(fmt, sums(fmt, x, q, scale)[0], scale, bias)


def bits(t):
    return t.contiguous().view(torch.int16)
