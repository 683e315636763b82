"""torch-CPU restatement of the NVFP4 arithmetic contracts (e2m1 codes, one e4m3 scale per 1 x 16 block, an optional fp32 per-tensor
scale p).  TEST INFRASTRUCTURE ONLY.  Paths relative to the reference torchao tree; pinned against tests/golden/nvfp4.npz, which
tests/golden/make_golden_nvfp4.py writes from the reference.

  cast        prototype/mx_formats/nvfp4_tensor.py:772-854 (nvfp4_quantize), :756-769 (per_tensor_amax_to_scale = amax / 2688)
              block_scale = amax / 6;  s8 = e4m3(clamp(block_scale [/ p], 2^-6, 448));  r = 1 / f32(s8)  [(1 / p) / f32(s8)];
              code = e2m1_rne(clamp(x r, -6, 6)), element 2i in the low nibble of byte i -- every step one fp32 operation
  dequantize  :199-257   s32 = p f32(s8) (f32(s8) without p);  v = f32(code) s32;  round to the output dtype
  weight-only :593-596   w = bf16(dequantize);  y = bf16(sum_k x w + bias): fp32 sum, bias inside the one rounding
  dynamic     :487-578   acc = sum_k (a_code a_s8)(b_code b_s8);  no per-tensor scale: y = bf16(acc + bias);  otherwise t = bf16(acc),
              u = bf16(f32(t) f32(bf16(P))), P = pa pb (fp32) or the one present, y = bf16(f32(u) + f32(bias))

The sums over k are taken in float64 and rounded to fp32 (the oracle's rounding, _parity.oracle_round).  Works on any device.
"""
import torch

E2M1_VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
E4M3_EPS = 2.0 ** -6  # torch.finfo(torch.float8_e4m3fn).tiny
BLOCK = 16


def bits(t):
    return t.contiguous().view(torch.int16)


def _bf16(v):
    return v.to(torch.float32).to(torch.bfloat16)


def e2m1_codes(v):
    """fp32 -> e2m1 code (uint8 0..15), round to nearest even, saturating at 6; the sign bit is kept (-0.0 is code 8).  A NaN gives the
    reference's code, which depends on its mantissa bits (custom_fp_utils._f32_to_floatx_unpacked takes the normal branch: the magic-adder
    rounding of the bit pattern): 4 for 0x7FF00000 (what f32(e4m3 NaN) and everything multiplied by it is on the CPU), 3 for 0x7FC00000."""
    v = v.to(torch.float32)
    a = v.abs()
    c = torch.zeros(v.shape, dtype=torch.uint8, device=v.device)
    # ties go to the even code: 0.25 -> 0, 0.75 -> 1.0, 1.25 -> 1.0, 1.75 -> 2.0, 2.5 -> 2.0, 3.5 -> 4.0, 5.0 -> 4.0
    for hit in (a > 0.25, a >= 0.75, a > 1.25, a >= 1.75, a > 2.5, a >= 3.5, a > 5.0):
        c += hit.to(torch.uint8)
    ab = v.view(torch.int32).to(torch.int64) & 0x7FFFFFFF
    nan_code = (((ab + 0xC11FFFFF + ((ab >> 22) & 1)) & 0xFFFFFFFF) >> 22) & 0x7
    c = torch.where(torch.isnan(v), nan_code.to(torch.uint8), c)
    sign = (v.view(torch.int32) < 0).to(torch.uint8) * 8
    return c | sign


def amax_scale(x):
    """per_tensor_amax_to_scale(torch.max(torch.abs(x)))"""
    return torch.max(torch.abs(x)).to(torch.float32) / 2688.0


def cast(x, p=None):
    """bf16 [R, C] -> (codes uint8 [R, C/2], scale bytes uint8 [R, C/16]); p: fp32 0-dim tensor or None."""
    R, C = x.shape
    v = x.to(torch.float32).reshape(R, C // BLOCK, BLOCK)
    bs = v.abs().amax(dim=-1) / 6.0
    if p is not None:
        p = p.to(torch.float32).reshape(())
        bs = bs / p
    s8 = torch.clamp(bs, min=E4M3_EPS, max=448.0).to(torch.float8_e4m3fn)
    sf = s8.to(torch.float32)
    r = (1.0 / sf) if p is None else (1.0 / p) / sf
    scaled = torch.clamp(v * r.unsqueeze(-1), -6.0, 6.0).reshape(R, C)
    c = e2m1_codes(scaled)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).contiguous(), s8.view(torch.uint8).contiguous()


def unpack(codes):
    """[R, C/2] bytes -> [R, C] codes"""
    return torch.stack([codes & 0xF, codes >> 4], dim=-1).reshape(codes.shape[0], codes.shape[1] * 2)


def values(codes):
    lut = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=codes.device)
    return lut[unpack(codes).long()]


def scales32(scale, p=None):
    s = scale.view(torch.float8_e4m3fn).to(torch.float32)
    return s if p is None else p.to(torch.float32).reshape(()) * s


def dequantize(codes, scale, p=None, dtype=torch.bfloat16):
    v = values(codes)
    R, C = v.shape
    return (v.reshape(R, C // BLOCK, BLOCK) * scales32(scale, p).unsqueeze(-1)).reshape(R, C).to(dtype)


# ---- weight-only linear ---------------------------------------------------------------------------------------------------------------
def wo_sums(x, codes, scale, p=None):
    """(m64, S): the float64 sum over k of x bf16(dequantize(w)) and the float64 sum of absolute products, [M, N]."""
    w = dequantize(codes, scale, p).to(torch.float64)
    xd = x.to(torch.float64)
    return xd @ w.t(), xd.abs() @ w.abs().t()


def wo_chain(m, bias=None):
    v = m.to(torch.float32)
    if bias is not None:
        v = v + bias.to(torch.bfloat16).to(torch.float32)
    return v.to(torch.bfloat16)


def wo_linear(x, codes, scale, p=None, bias=None):
    return wo_chain(wo_sums(x, codes, scale, p)[0], bias)


# ---- dynamic (codes x codes) linear ---------------------------------------------------------------------------------------------------
def mm_sums(a, a_scale, b, b_scale):
    ad = dequantize(a, a_scale, None, torch.float64)  # code x block scale: exact
    bd = dequantize(b, b_scale, None, torch.float64)
    return ad @ bd.t(), ad.abs() @ bd.abs().t()


def mm_P(pa, pb):
    if pa is not None and pb is not None:
        return pa.to(torch.float32).reshape(()) * pb.to(torch.float32).reshape(())
    return pa if pa is not None else pb


def mm_chain(m, pa=None, pb=None, bias=None):
    P = mm_P(pa, pb)
    v = m.to(torch.float32)
    if P is None:
        if bias is not None:
            v = v + bias.to(torch.bfloat16).to(torch.float32)
        return v.to(torch.bfloat16)
    t = v.to(torch.bfloat16)
    u = _bf16(t.to(torch.float32) * P.to(torch.float32).reshape(()).to(torch.bfloat16).to(torch.float32))
    if bias is not None:
        u = _bf16(u.to(torch.float32) + bias.to(torch.bfloat16).to(torch.float32))
    return u


def mm(a, a_scale, b, b_scale, pa=None, pb=None, bias=None):
    return mm_chain(mm_sums(a, a_scale, b, b_scale)[0], pa, pb, bias)


def dynamic_linear(x, b, b_scale, pb=None, pa=None, dynamic=False, bias=None):
    """the dynamic linear from a bf16 activation: per-tensor scale (dynamic: from the amax), cast, GEMM"""
    pa = amax_scale(x) if dynamic else pa
    a, a_scale = cast(x, pa)
    return mm(a, a_scale, b, b_scale, pa, pb, bias)


def unswizzle(blocked, rows, cols):
    """to_blocked's 128 x 4 layout (prototype/mx_formats/utils.py:31-72) back to row-major [rows, cols], element by element."""
    flat = blocked.reshape(-1)
    cb = (cols + 3) // 4
    out = torch.empty((rows, cols), dtype=flat.dtype)
    for r in range(rows):
        for c in range(cols):
            out[r, c] = flat[((r // 128) * cb + c // 4) * 512 + (r % 32) * 16 + (r % 128 // 32) * 4 + c % 4]
    return out
