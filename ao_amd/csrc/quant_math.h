// The 8-bit arithmetic at both ends of a linear, the reference's op sequence element for element.  Per-row activation quantisation,
// shared by the stand-alone casts (quant_kernels.hip) and the fused dynamic-quant linears (dyn8_kernels.hip):
//   int8 : scale = f32(max(bf16(amax / 127.5), bf16(f32_eps)));  q = clamp(rint(x * (1/scale)), -128, 127)
//          (int8_tensor.py:191-230, quant_primitives.py:1534-1583, :463-485)
//   fp8  : scale = f32(bf16(amax / 448));  q = e4m3_rne(clamp(f32(x) / scale, -448, 448))
//          (float8_tensor.py:167-253, quant_primitives.py:2192-2212, 2271-2287)
// and the rowwise output epilogue, shared by every int8 / fp8 GEMM kernel and the stand-alone scale epilogues (epilogue8 below).
#pragma once
#include "common.h"

namespace ao {

// NaN-propagating max like torch.amax: fmaxf drops NaN, so track it separately
__device__ __forceinline__ float amax8(const u32x4& v, bool& has_nan) {
  float m = 0.f;
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = fabsf(bf16_lo_to_f32(w[i])), b = fabsf(bf16_hi_to_f32(w[i]));
    has_nan |= (a != a) | (b != b);
    m = fmaxf(m, fmaxf(a, b));
  }
  return m;
}

__device__ __forceinline__ float int8_row_scale(float amax) {
  const float s = round_bf16(amax / 127.5f);
  return fmaxf(s, 1.1920928955078125e-07f);  // fp32 eps, exactly representable in bf16
}
// 8 bf16 -> 8 int8 (two dwords); inv = 1 / scale
__device__ __forceinline__ u32x2 int8_quant8(const u32x4& v, float inv) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t out[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = fminf(fmaxf(rintf(bf16_lo_to_f32(w[j]) * inv), -128.f), 127.f);
    const float b = fminf(fmaxf(rintf(bf16_hi_to_f32(w[j]) * inv), -128.f), 127.f);
    const uint32_t pa = (uint32_t)(int)a & 0xffu, pb = (uint32_t)(int)b & 0xffu;
    out[j >> 1] |= (pa | (pb << 8)) << ((j & 1) * 16);
  }
  return u32x2{out[0], out[1]};
}
// the zero-point form (asymmetric / static activations, quant_primitives.py:463-485): q = clamp(rint(x * inv) + zp, -128, 127).  Not
// int8_quant8 with zp = 0: + 0.0f turns a -0.0 into +0.0, so the symmetric form would gain an add.
__device__ __forceinline__ u32x2 int8_quant8_zp(const u32x4& v, float inv, float zp) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t out[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = fminf(fmaxf(rintf(bf16_lo_to_f32(w[j]) * inv) + zp, -128.f), 127.f);
    const float b = fminf(fmaxf(rintf(bf16_hi_to_f32(w[j]) * inv) + zp, -128.f), 127.f);
    const uint32_t pa = (uint32_t)(int)a & 0xffu, pb = (uint32_t)(int)b & 0xffu;
    out[j >> 1] |= (pa | (pb << 8)) << ((j & 1) * 16);
  }
  return u32x2{out[0], out[1]};
}

// an activation pre-scale (AWQ / SmoothQuant: `x * act_pre_scale`, a bf16 tensor op) folded into a cast: 8 bf16 x 8 bf16 -> 8 bf16,
// t = bf16_rne(f32(x) * f32(pre)).  Two 8-bit significands give a product of 16 bits, exact in fp32, so the rounding to bf16 is the only
// one, as in torch's bf16 multiply (fp32 opmath, one conversion).  The casts above then run on t as they do on x (quant_kernels.hip, load8).
__device__ __forceinline__ u32x4 prescale8(const u32x4& x, const u32x4& pre) {
  const uint32_t a[4] = {x.x, x.y, x.z, x.w}, b[4] = {pre.x, pre.y, pre.z, pre.w};
  uint32_t t[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    t[j] = pack_bf16x2(mul_f32_rn(bf16_lo_to_f32(a[j]), bf16_lo_to_f32(b[j])), mul_f32_rn(bf16_hi_to_f32(a[j]), bf16_hi_to_f32(b[j])));
  return u32x4{t[0], t[1], t[2], t[3]};
}

__device__ __forceinline__ float fp8_row_scale(float amax) { return round_bf16(amax / 448.0f); }
__device__ __forceinline__ uint32_t cvt4_e4m3(float a, float b, float c, float d) {
  uint32_t r = 0;
  r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, r, false);
  r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
  return r;
}
// two values: the codes in the low 16 bits
__device__ __forceinline__ uint32_t cvt2_e4m3(float a, float b) { return __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0u, false) & 0xffffu; }
__device__ __forceinline__ float clamp448(float v) {
  // torch.clamp propagates NaN; fminf/fmaxf would not
  return (v != v) ? v : fminf(fmaxf(v, -448.f), 448.f);
}
// 8 bf16 -> 8 e4m3 (two dwords).  The reference divides (tensor_fp32 / scale).  Here: one IEEE reciprocal per call and a
// residual-corrected product per element, q0 = x r;  q = fma(fma(-q0, s, x), r, q0), which gives the SAME e4m3 codes: when x / s
// is exactly representable (the only way it can sit on an e4m3 rounding boundary or on the 448 clamp: x and s are bf16-valued)
// the correction recovers it exactly; otherwise it is within an ulp of the correctly rounded quotient and at least 2^-13
// (relative) away from any boundary.  tests/test_oracle_variants.py checks every bf16 x against scales over 200 binades.  Scales
// whose reciprocal would overflow or go denormal take the division.
__device__ __forceinline__ u32x2 fp8_quant8(const u32x4& v, float s) {
  float f[8] = {bf16_lo_to_f32(v.x), bf16_hi_to_f32(v.x), bf16_lo_to_f32(v.y), bf16_hi_to_f32(v.y),
                bf16_lo_to_f32(v.z), bf16_hi_to_f32(v.z), bf16_lo_to_f32(v.w), bf16_hi_to_f32(v.w)};
  if (s > 0x1p-100f && s < 0x1p100f) {  // uniform per row
    const float r = 1.0f / s;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float q0 = f[j] * r;
      const float q = __builtin_fmaf(__builtin_fmaf(-q0, s, f[j]), r, q0);
      f[j] = clamp448((fabsf(q0) < INFINITY && q0 != 0.0f) ? q : q0);  // inf / NaN / signed zero pass through like the division
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = clamp448(f[j] / s);
  }
  return u32x2{cvt4_e4m3(f[0], f[1], f[2], f[3]), cvt4_e4m3(f[4], f[5], f[6], f[7])};
}

// ---- float8 TRAINING cast (fp8_train_kernels.hip): torchao/float8, not the inference cast above -------------------------------------
//   scale = f32(448 / max(f64(amax), 1e-12)): divided in float64 and rounded once to fp32 (float8_utils.py:31-53); with
//   round_scales_to_power_of_2, exp2(floor(log2(scale))) (:244-246) -- the mantissa bits cleared: every scale this formula gives from a
//   bf16 amax is a normal fp32 (448 / 3.4e38 = 1.3e-36 .. 448 / 1e-12 = 4.5e14).
//   q = e4m3_rne(clamp(f32(x) * scale, -448, 448))  (float8_training_tensor.py:153-154, float8_utils.py:118-139).  The clamp is live:
//   without the power-of-two rounding amax * scale can round above 448.
//   The GEMM multiplies by 1 / scale, an IEEE fp32 division (float8_ops.py:44-45).
__device__ __forceinline__ float fp8_train_scale(float amax, bool pow2) {
  const float s = (float)(448.0 / fmax((double)amax, 1e-12));
  return pow2 ? bits_to_f32(f32_to_bits(s) & 0xff800000u) : s;
}
__device__ __forceinline__ float fp8_train_q(float x, float s) { return clamp448(x * s); }
// 8 bf16 of one row -> 8 e4m3 codes (two dwords) under the row's scale
__device__ __forceinline__ u32x2 fp8_train_quant8(const u32x4& v, float s) {
  return u32x2{cvt4_e4m3(fp8_train_q(bf16_lo_to_f32(v.x), s), fp8_train_q(bf16_hi_to_f32(v.x), s), fp8_train_q(bf16_lo_to_f32(v.y), s),
                         fp8_train_q(bf16_hi_to_f32(v.y), s)),
               cvt4_e4m3(fp8_train_q(bf16_lo_to_f32(v.z), s), fp8_train_q(bf16_hi_to_f32(v.z), s), fp8_train_q(bf16_lo_to_f32(v.w), s),
                         fp8_train_q(bf16_hi_to_f32(v.w), s))};
}

// ---- rowwise output epilogue: the fp32 value the caller rounds to bf16 at its store -----------------------------------------------
//   int8 : t = bf16(f32(c) * sx[m]);  y = bf16(f32(t) * sw[n] (+ bias))   (int8_tensor.py:315-359)
//   fp8  : y = bf16(c * sa[m] * sb[n] (+ bias))                           (float8/inference.py:104-123)
// The int8 product t * sw and the bias add are two tensor ops: mul_f32_rn keeps them from contracting into one v_fma_f32.
// c is the accumulator already converted to fp32 by the caller ((float) of the int32 sum for int8): converting it in here
// reorders the K loop of gemm8_dma_kernel<0, ...>.  Kernels that load the bias at the store, only where there is one, call without
// it and add it after: the same fp32 add, and passing it in changed their branch layout.
// int8's last step alone: the asymmetric epilogue (quant_kernels.hip) applies its zero-point correction to t first.
__device__ __forceinline__ float int8_out(float t, float sc, bool has_bias = false, float bias = 0.f) {
  float v = mul_f32_rn(t, sc);
  if (has_bias) v += bias;
  return v;
}
template <bool INT8>
__device__ __forceinline__ float epilogue8(float c, float sr, float sc, bool has_bias = false, float bias = 0.f) {
  if (INT8) return int8_out(round_bf16(c * sr), sc, has_bias, bias);
  float v = c * sr * sc;
  if (has_bias) v += bias;
  return v;
}

// ---- weight-only linears (wo8_kernels.hip): bf16 activation x 8-bit weight ----------------------------------------------------------
// 16 codes -> 16 bf16 weights (w0: codes 0..7, w1: 8..15), the operand the bf16 MFMA multiplies.
//   int8 : bf16(q), exact (int8_tensor.py:347-351: qdata.t().to(bf16))
//   e4m3 : bf16(f32(q) * s), the fp32 product rounded to fp32 and then to bf16 (float8_tensor.py:255-275 dequantize, :466)
template <bool INT8>
__device__ __forceinline__ void wo8_weight16(const u32x4& q, float s, u32x4& w0, u32x4& w1) {
  const uint32_t c[4] = {q.x, q.y, q.z, q.w};
  uint32_t o[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (INT8) {
      const int v = (int)c[i];
      o[2 * i] = pack_bf16x2((float)((v << 24) >> 24), (float)((v << 16) >> 24));
      o[2 * i + 1] = pack_bf16x2((float)((v << 8) >> 24), (float)(v >> 24));
    } else {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], true);
      o[2 * i] = pack_bf16x2(lo.x * s, lo.y * s);
      o[2 * i + 1] = pack_bf16x2(hi.x * s, hi.y * s);
    }
  }
  w0 = u32x4{o[0], o[1], o[2], o[3]};
  w1 = u32x4{o[4], o[5], o[6], o[7]};
}
// The output epilogue: the fp32 value the caller rounds to bf16 at its store (c: the fp32 sum).
//   int8 : t = bf16(c);  u = bf16(f32(t) * f32(bf16(s)));  y = bf16(f32(u) + bias)   (int8_tensor.py:352-359: scale.to(m.dtype), y += bias)
//   e4m3 : t = bf16(c);  y = bf16(f32(t) + bias)                                      (float8_tensor.py:466-468; s went into the weights)
// Three roundings for int8, not epilogue8's one: every step is a bf16 tensor op in the reference.
template <bool INT8>
__device__ __forceinline__ float wo8_out(float c, float s, bool has_bias = false, float bias = 0.f) {
  float v = round_bf16(c);
  if (INT8) v = round_bf16(mul_f32_rn(v, round_bf16(s)));
  if (has_bias) v += bias;
  return v;
}

// ---- blockwise float8 linears (fp8_block_kernels.hip): 1 x 128 activation blocks, 128 x 128 weight blocks ----------------------------
// One K block onto the accumulator of a lane's four rows (kernels.py:85-97: accumulator += tl.dot(a, b) * a_s[:, None] * b_s[None, :]):
//   acc[r] += (p[r] * a_s[r]) * b_s, two products and a sum in fp32, each rounded on its own -- the chain tests/fp8_block_ref.py restates
// in plain fp32, so none of them may contract into a v_fma_f32.  p: the block's 128-k MFMA onto a zero accumulator.
__device__ __forceinline__ f32x4 fp8_block_acc(f32x4 acc, f32x4 p, f32x4 a_s, float b_s) {
#pragma clang fp contract(off)
  const f32x4 t = p * a_s;
  const f32x4 u = t * b_s;
  return acc + u;
}
// The output: t = bf16(acc);  y = bf16(f32(t) + bias[n]) -- rounded to bf16 BEFORE the bias (float8_tensor.py:445-447: the GEMM returns
// bf16, the bias is added to that tensor).  The fp32 value the caller rounds to bf16 at its store.
__device__ __forceinline__ float fp8_block_out(float acc, bool has_bias = false, float bias = 0.f) {
  float v = round_bf16(acc);
  if (has_bias) v += bias;
  return v;
}

// ---- MXFP8 (to_mx, prototype/mx_formats/mx_tensor.py:228-409) --------------------------------------------------------------------
// E8M0 scale exponent of one 32-block from its amax (:255-330; RCEIL :111-129, :161-225) and the reciprocal 2^(127 - e) built from the
// E8M0 byte 254 - e (:132-158).  MODE: AO_MX_SCALE_FLOOR (0) / AO_MX_SCALE_RCEIL (1).
template <int MODE>
__device__ __forceinline__ uint32_t mx_block_exponent(float m, bool finite) {
  uint32_t e;
  if (MODE == 1) {
    // descale = amax * (1/448) in fp32; its value rounded up to a power of two
    const uint32_t bits = f32_to_bits(m * (1.0f / 448.0f));
    const uint32_t be = (bits >> 23) & 0xffu, mant = bits & 0x7fffffu;
    const bool up = (be == 0) ? (mant > 0x400000u) : (mant != 0);
    e = be + (up ? 1u : 0u);
  } else {
    // floor(log2(amax)) - 8, clamped to [-127, 128], biased
    const int ex = (int)((f32_to_bits(m) >> 23) & 0xffu) - 127 - 8;
    e = (uint32_t)(min(max(ex, -127), 128) + 127);
  }
  return finite ? e : 255u;
}
__device__ __forceinline__ float mx_reciprocal(uint32_t e) {
  const uint32_t re = (254u - e) & 0xffu;
  uint32_t rbits = re << 23;
  if (re == 0u) rbits = 0x00400000u;    // 2^-127 as an fp32 subnormal
  if (re == 255u) rbits = 0x7F800001u;  // NaN
  return bits_to_f32(rbits);
}
// 8 bf16 -> 8 e4m3 codes of a block whose E8M0 exponent is e (to_mx's data_hp * reciprocal, then the saturating cast)
template <int MODE>
__device__ __forceinline__ u32x2 mx_encode8(const u32x4& v, uint32_t e) {
  const float r = mx_reciprocal(e);
  float f[8] = {bf16_lo_to_f32(v.x), bf16_hi_to_f32(v.x), bf16_lo_to_f32(v.y), bf16_hi_to_f32(v.y),
                bf16_lo_to_f32(v.z), bf16_hi_to_f32(v.z), bf16_lo_to_f32(v.w), bf16_hi_to_f32(v.w)};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    f[j] *= r;
    if (MODE == 0) f[j] = clamp448(f[j]);  // eager saturation (torch < 2.13), :361-373
  }
  return u32x2{cvt4_e4m3(f[0], f[1], f[2], f[3]), cvt4_e4m3(f[4], f[5], f[6], f[7])};
}
// The 1 x 32 cast of one block by FOUR ADJACENT LANES (lane & 3 = the block's quarter: 8 bf16 each): block amax across the four lanes,
// the E8M0 exponent (returned in e, the same in all four), 8 e4m3 codes of this lane's quarter.  One definition for the stand-alone cast
// (quant_kernels.hip: mxfp8_quant_kernel) and the cast fused into the grouped GEMM's A-fill (rb8_kernels.hip): the same bits by construction.
template <int MODE>
__device__ __forceinline__ u32x2 mx_cast8(const u32x4& v, uint32_t& e) {
  bool has_nan = false;
  float m = amax8(v, has_nan);
  m = fmaxf(m, __shfl_xor(m, 1));
  m = fmaxf(m, __shfl_xor(m, 2));
  uint32_t nanbits = has_nan ? 1u : 0u;
  nanbits |= __shfl_xor(nanbits, 1);
  nanbits |= __shfl_xor(nanbits, 2);
  e = mx_block_exponent<MODE>(m, (nanbits == 0u) && (m < INFINITY));
  return mx_encode8<MODE>(v, e);
}
// The same cast of one block by the SIXTEEN LANES OF A DPP ROW, two adjacent bf16 each (the register layout of the colwise kernel, whose
// lanes hold two columns): the block amax across the row (common.h: row16_max), the exponent (in e, the same in all sixteen), this lane's two
// codes in the low 16 bits.  A NaN rides the reduction as +inf: either makes the block non-finite, the only thing mx_cast8 asks of them.
template <int MODE>
__device__ __forceinline__ uint32_t mx_cast2(uint32_t v, uint32_t& e) {
  const float lo = bf16_lo_to_f32(v), hi = bf16_hi_to_f32(v);
  const float a = fabsf(lo), b = fabsf(hi);
  const float m = row16_max(((a != a) | (b != b)) ? INFINITY : fmaxf(a, b));
  e = mx_block_exponent<MODE>(m, m < INFINITY);
  const float r = mx_reciprocal(e);
  float f0 = lo * r, f1 = hi * r;
  if (MODE == 0) {  // eager saturation, as in mx_encode8
    f0 = clamp448(f0);
    f1 = clamp448(f1);
  }
  return cvt2_e4m3(f0, f1);
}

// ---- MXFP4 (to_mx(x, float4_e2m1fn_x2, 32, mode)) ---------------------------------------------------------------------------------
// Block exponent (F4_E2M1_MAX_POW2 = 2; RCEIL: descale = amax * f32(1/6) rounded up to a power of two, :161-225) and the e2m1 code of one
// scaled value by the integer steps of custom_fp_utils._f32_to_floatx_unpacked(x, 2, 1): |x| >= 6 saturates to 7; |x| < 1 is rounded
// by the fp32 add x + 2^22 (RNE at a step of 0.5); otherwise the mantissa is rounded to one bit by the magic-adder form (a NaN takes
// this branch, like the reference's).  The sign bit is kept, -0 included.
template <int MODE>
__device__ __forceinline__ uint32_t mxfp4_block_exponent(float m, bool finite) {
  uint32_t e;
  if (MODE == 1) {
    const uint32_t bits = f32_to_bits(m * (1.0f / 6.0f));
    const uint32_t be = (bits >> 23) & 0xffu, mant = bits & 0x7fffffu;
    const bool up = (be == 0) ? (mant > 0x400000u) : (mant != 0);
    e = be + (up ? 1u : 0u);
  } else {
    const int ex = (int)((f32_to_bits(m) >> 23) & 0xffu) - 127 - 2;
    e = (uint32_t)(min(max(ex, -127), 128) + 127);
  }
  return finite ? e : 255u;
}
__device__ __forceinline__ uint32_t e2m1_code(uint32_t bits) {
#pragma clang fp contract(off)
  const uint32_t sign = (bits >> 28) & 8u;
  const uint32_t a = bits & 0x7fffffffu;
  const float x = bits_to_f32(a);
  uint32_t c;
  if (x >= 6.0f) {
    c = 7u;
  } else if (x < 1.0f) {
    c = (f32_to_bits(x + 0x1p22f) - (149u << 23)) & 0xffu;
  } else {
    c = ((a + (0xC1000000u + 0x1FFFFFu) + ((a >> 22) & 1u)) >> 22) & 0xffu;  // ((1 - 127) << 23) + magic adder, mod 2^32
  }
  return c | sign;
}
// The 1 x 32 cast of one block held by ONE lane (32 bf16 in four 16-byte pieces): E8M0 exponent in e, 32 codes packed two per byte (element
// 2i in the low nibble, pack_uint4).  One definition for the stand-alone cast and the cast fused into the MX linear's A operand.
// Non-finite blocks (e = 255) multiply by the NaN reciprocal 0x7F800001: the reference's products are that NaN quieted (0x7FC00001) for
// every element, NaN elements included, so all 32 codes are e2m1_code(0x7FC00001) = 3 -- taken here from the bits, not from whichever
// NaN operand the hardware multiply would propagate.
template <int MODE>
__device__ __forceinline__ u32x4 mx_cast4(const u32x4 (&v)[4], uint32_t& e) {
  bool has_nan = false;
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) m = fmaxf(m, amax8(v[i], has_nan));
  e = mxfp4_block_exponent<MODE>(m, !has_nan && m < INFINITY);
  const float r = mx_reciprocal(e);
  uint32_t out[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
    uint32_t o = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t xb = (j & 1) ? (w[j >> 1] & 0xffff0000u) : (w[j >> 1] << 16);
      const uint32_t pb = (e == 255u) ? 0x7FC00001u : f32_to_bits(bits_to_f32(xb) * r);
      o |= e2m1_code(pb) << (4 * j);
    }
    out[i] = o;
  }
  return u32x4{out[0], out[1], out[2], out[3]};
}

// ---- NVFP4 (nvfp4_kernels.hip): e2m1 codes, one e4m3 scale per 1 x 16 block, an optional fp32 per-tensor scale p -----------------------
// The contracts of prototype/mx_formats/nvfp4_tensor.py, each stated once:
//   cast (nvfp4_quantize, :772-854), per block, in fp32:  block_scale = amax / 6;
//     no p: s8 = e4m3(clamp(block_scale, 2^-6, 448));      r = 1.0 / f32(s8)
//     p   : s8 = e4m3(clamp(block_scale / p, 2^-6, 448));  r = (1.0 / p) / f32(s8)
//     code = f32_to_f4_unpacked(clamp(x r, -6, 6)) (e2m1_code above), element 2i in the low nibble of byte i (pack_uint4)
//   per_tensor_amax_to_scale (:756-769): amax / 2688
//   dequantize (:199-257): s32 = p f32(s8) (f32(s8) without p);  v = f32(code) s32;  round v to the output dtype -- with a p that is
//     not a power of two both fp32 products round, and both roundings are kept
//   weight-only linear (nvfp4_linear, :593-596): w = bf16(dequantize);  y = bf16(sum_k x w + bias), fp32 accumulation, ONE rounding
//   dynamic linear (_addmm_nvfp4_dispatch, :487-578): acc = sum_k (a_code a_s8)(b_code b_s8) in fp32 -- code x block scale is exact in
//     bf16 (2 + 4 significand bits), so the bf16 MFMA multiplies the products a native FP4 unit would.  No per-tensor scale:
//     y = bf16(acc + bias).  Otherwise t = bf16(acc);  u = bf16(f32(t) f32(bf16(P)));  y = bf16(f32(u) + f32(bias)), P = pa pb (fp32
//     product) or the one scale that is present.
constexpr float kE4M3Eps = 0.015625f;  // torch.finfo(float8_e4m3fn).tiny

// f32 of one e4m3 scale byte
__device__ __forceinline__ float e4m3_byte_to_f32(uint32_t b) {
  const f32x2 v = __builtin_amdgcn_cvt_pk_f32_fp8((int)b, false);
  return v.x;
}
// dequantize's scale: p f32(s8), the fp32 product rounded on its own
__device__ __forceinline__ float nvfp4_scale32(uint32_t s8, bool has_p, float p) {
  const float s = e4m3_byte_to_f32(s8);
  return has_p ? mul_f32_rn(p, s) : s;
}
// 16 codes of one block (8 bytes) -> 16 bf16 (w0: elements 0..7, w1: 8..15) = bf16(f32(code) s32).  An e2m1 nibble seee placed in an e4m3
// byte as s00ee.m00 reads as the e2m1 value / 64, subnormals included, so the hardware e4m3 convert and an exact x 64 give f32(code).
__device__ __forceinline__ void nvfp4_block16(u32x2 q, float s32, u32x4& w0, u32x4& w1) {
#pragma clang fp contract(off)
  const uint32_t c[2] = {q.x, q.y};
  uint32_t o[8];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t ev = ((c[i] & 0x08080808u) << 4) | ((c[i] & 0x07070707u) << 2);          // elements 0, 2, 4, 6 of the dword
    const uint32_t od = (c[i] & 0x80808080u) | (((c[i] >> 4) & 0x07070707u) << 2);           // elements 1, 3, 5, 7
    const f32x2 e01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)ev, false), e23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)ev, true);
    const f32x2 o01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)od, false), o23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)od, true);
    o[4 * i + 0] = pack_bf16x2((e01.x * 64.0f) * s32, (o01.x * 64.0f) * s32);
    o[4 * i + 1] = pack_bf16x2((e01.y * 64.0f) * s32, (o01.y * 64.0f) * s32);
    o[4 * i + 2] = pack_bf16x2((e23.x * 64.0f) * s32, (o23.x * 64.0f) * s32);
    o[4 * i + 3] = pack_bf16x2((e23.y * 64.0f) * s32, (o23.y * 64.0f) * s32);
  }
  w0 = u32x4{o[0], o[1], o[2], o[3]};
  w1 = u32x4{o[4], o[5], o[6], o[7]};
}
__device__ __forceinline__ float clamp6(float v) { return (v != v) ? v : fminf(fmaxf(v, -6.f), 6.f); }  // torch.clamp keeps NaN
// The 1 x 16 cast of one block held by ONE lane (16 bf16 in two 16-byte pieces): the e4m3 scale byte in s8, 16 codes packed two a byte.
// A block that holds a NaN, or any block under a NaN p (the dynamic amax of an activation that holds one), has the scale byte 0x7F and
// every product NaN.  The reference's codes then come from that NaN's mantissa bits: f32(e4m3 NaN) is 0x7FF00000 on its CPU run and so is
// every product, code 4; under a NaN p the reciprocal is 1 / p = 0x7FC00000, code 3.  Taken here from the case, not from whichever NaN the
// hardware multiply would propagate.  (A zero or infinite p is outside the contract.)
__device__ __forceinline__ u32x2 nvfp4_cast16(const u32x4 (&v)[2], bool has_p, float p, uint32_t& s8) {
#pragma clang fp contract(off)
  bool has_nan = false;
  float m = fmaxf(amax8(v[0], has_nan), amax8(v[1], has_nan));
  if (has_nan) m = bits_to_f32(0x7FC00000u);
  float bs = m / 6.0f;
  if (has_p) bs = bs / p;
  const float cl = (bs != bs) ? bs : fminf(fmaxf(bs, kE4M3Eps), 448.0f);
  s8 = (cl != cl) ? 0x7Fu : (cvt4_e4m3(cl, 0.f, 0.f, 0.f) & 0xffu);
  if (s8 == 0x7Fu) return (has_p && p != p) ? u32x2{0x33333333u, 0x33333333u} : u32x2{0x44444444u, 0x44444444u};
  const float sf = e4m3_byte_to_f32(s8);
  const float r = has_p ? (1.0f / p) / sf : 1.0f / sf;
  uint32_t out[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
    uint32_t o = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t xb = (j & 1) ? (w[j >> 1] & 0xffff0000u) : (w[j >> 1] << 16);
      o |= e2m1_code(f32_to_bits(clamp6(bits_to_f32(xb) * r))) << (4 * j);
    }
    out[i] = o;
  }
  return u32x2{out[0], out[1]};
}
// The outputs: the fp32 value the caller rounds to bf16 at its store (c: the fp32 sum).
__device__ __forceinline__ float nvfp4_wo_out(float c, bool has_bias, float bias) { return has_bias ? c + bias : c; }
// P of the dynamic linear from the two device pointers (null: none); has_P false when neither is present
__device__ __forceinline__ float nvfp4_P(const float* pa, const float* pb, bool& has_P) {
  has_P = pa != nullptr || pb != nullptr;
  if (pa != nullptr && pb != nullptr) return mul_f32_rn(*pa, *pb);
  return pa != nullptr ? *pa : (pb != nullptr ? *pb : 1.0f);
}
__device__ __forceinline__ float nvfp4_mm_out(float c, bool has_P, float P, bool has_bias, float bias) {
  if (!has_P) return has_bias ? c + bias : c;
  const float u = round_bf16(mul_f32_rn(round_bf16(c), round_bf16(P)));
  return has_bias ? u + bias : u;
}

// ---- NVFP4 training (nvfp4_train_kernels.hip): the casts of prototype/moe_training/nvfp4_training ---------------------------------------
// TransformerEngine's scale chain as test/prototype/moe_training/nvfp4_training/nvfp4_reference.py states it and
// hadamard_utils._nvfp4_quantize implements it -- not nvfp4_quantize's above: the scale is rounded ONCE, the block scale has no lower
// clamp, and the per-tensor scale is folded into an encode scale.  Every step one fp32 operation, the divisions correctly rounded:
//   global   S_enc = min(2688 / amax, FLT_MAX);  S_enc = 1 if amax == 0 or the quotient is 0;  S_dec_global = 1 / S_enc
//   block    s8 = e4m3(min(block_amax (S_enc (1/6)), 448)): the inner product rounded once, NO lower clamp (a zero block, or one that
//            underflows e4m3, has the scale byte 0)
//   encode   enc = min(1 / (f32(s8) S_dec_global), FLT_MAX);  scaled = clamp(x enc, -6, 6)
//   RTNE     e2m1_code above, element 2i in the low nibble of byte i; the sign bit is kept (-0 is code 8)
//   RHT      for 16 consecutive elements a_0..a_15, the sign vector s and the Sylvester matrix: y_j = bf16(1/4 sum_i s_i a_i (-1)^popcount(i & j)),
//            the sum in fp32 by a butterfly of four add/sub stages (i ^ 1, i ^ 2, i ^ 4, i ^ 8).  The fp32 sum is exact in ANY order while
//            the 16 inputs' exponents span fewer than 12 binades (8 significand bits + 4 bits of growth + 12 < 24); outside that the
//            butterfly's order is this kernel's own and another order may round differently.  A zero sum is +0, also where every term
//            is -0: the reference's matrix product starts its accumulator at +0.
//   SR       (the reference draws Triton's Philox stream and rounds with PTX cvt.rs, neither reproducible here: this is this library's
//            own contract)  a = min(|scaled|, 6);  lo <= a <= hi the e2m1 magnitudes around a (on the grid lo = hi = a);
//            t = (a - lo) / (hi - lo), exact in fp32 (the steps are powers of two and the subtraction is exact);  the magnitude is hi iff
//            r16 < t 65536, else lo;  the sign is kept.  P(up) = ceil(t 2^16) / 2^16: the bias is below 2^-16 of a step.
//   bits     Philox4x32-10 with its published constants;  key = the two 32-bit halves of the int64 seed;  counter = (g_lo, g_hi,
//            offset & 0xFFFFFFFF, stream), g the index in the output's row-major order of the group of 8 consecutive codes (one packed
//            dword), stream 0 the row output and 1 the column output;  element j of the group takes bits 16 (j & 1) .. + 15 of output
//            word j >> 1.  The bytes depend only on (seed, offset), never on the grid.
// NaN and Inf inputs are outside the contract of the training casts.
constexpr float kF32Max = 3.4028234663852886e38f;

struct Nvfp4TrainGlobal {
  float s_enc_sixth;  // S_enc (1/6)
  float s_dec;        // 1 / S_enc
};
__device__ __forceinline__ Nvfp4TrainGlobal nvfp4_train_global(float amax) {
#pragma clang fp contract(off)
  float s_enc = fminf(2688.0f / amax, kF32Max);
  if (amax == 0.0f || s_enc == 0.0f) s_enc = 1.0f;
  return Nvfp4TrainGlobal{s_enc * (1.0f / 6.0f), 1.0f / s_enc};
}
// block amax -> the e4m3 scale byte in s8 and the encode scale
__device__ __forceinline__ float nvfp4_train_encode(float block_amax, const Nvfp4TrainGlobal& g, uint32_t& s8) {
#pragma clang fp contract(off)
  s8 = cvt4_e4m3(fminf(block_amax * g.s_enc_sixth, 448.0f), 0.f, 0.f, 0.f) & 0xffu;
  return fminf(1.0f / (e4m3_byte_to_f32(s8) * g.s_dec), kF32Max);
}
__device__ __forceinline__ float nvfp4_train_scaled(float x, float enc) {
#pragma clang fp contract(off)
  return fminf(fmaxf(x * enc, -6.0f), 6.0f);
}

struct Philox4 {
  uint32_t w[4];
};
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}
// the SR code of one scaled value (|scaled| <= 6) under 16 random bits
__device__ __forceinline__ uint32_t e2m1_code_sr(float scaled, uint32_t r16) {
#pragma clang fp contract(off)
  const uint32_t sign = (f32_to_bits(scaled) >> 28) & 8u;
  const float a = fminf(fabsf(scaled), 6.0f);
  uint32_t c;
  float t;
  if (a < 2.0f) {  // steps of 0.5: codes 0..3
    const float f = floorf(a * 2.0f);
    c = (uint32_t)f;
    t = a * 2.0f - f;
  } else if (a < 4.0f) {  // steps of 1: codes 4, 5
    const float f = floorf(a);
    c = (uint32_t)f + 2u;
    t = a - f;
  } else if (a < 6.0f) {  // one step of 2: code 6
    c = 6u;
    t = (a - 4.0f) * 0.5f;
  } else {
    c = 7u;
    t = 0.0f;
  }
  if ((float)r16 < t * 65536.0f) c += 1u;
  return c | sign;
}
// 16 signed values -> their randomized Hadamard transform, each rounded to bf16 (held as fp32); bit i of sign_mask set: s_i = -1
__device__ __forceinline__ void nvfp4_rht16(float (&a)[16], uint32_t sign_mask) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = bits_to_f32(f32_to_bits(a[i]) ^ (((sign_mask >> i) & 1u) << 31));
#pragma unroll
  for (int h = 1; h < 16; h <<= 1)
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((i & h) == 0) {
        const float u = a[i], v = a[i | h];
        a[i] = u + v;
        a[i | h] = u - v;
      }
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = round_bf16((a[i] + 0.0f) * 0.25f);  // (+ 0: a sum of -0 terms alone is +0, as from an accumulator)
}
// 16 values of one block -> 16 codes packed two a byte.  SR: g0 the index of the block's first group of 8 codes (the second is g0 + 1).
template <bool SR>
__device__ __forceinline__ u32x2 nvfp4_train_codes16(const float (&a)[16], float enc, uint64_t g0, uint32_t offset, uint32_t stream,
                                                     uint32_t k0, uint32_t k1) {
  uint32_t out[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    Philox4 rnd = {};
    if (SR) {
      const uint64_t g = g0 + h;
      rnd = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), offset, stream, k0, k1);
    }
    uint32_t o = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = nvfp4_train_scaled(a[8 * h + j], enc);
      const uint32_t c = SR ? e2m1_code_sr(v, (rnd.w[j >> 1] >> (16 * (j & 1))) & 0xffffu) : e2m1_code(f32_to_bits(v));
      o |= c << (4 * j);
    }
    out[h] = o;
  }
  return u32x2{out[0], out[1]};
}
// the scaled_mm epilogue of the training GEMMs: out = bf16(acc (pa pb)), the product of the two scales in fp32, ONE rounding, no bias
__device__ __forceinline__ float nvfp4_scaled_mm_out(float c, float P) { return mul_f32_rn(c, P); }

// ---- NF4 (nf4_kernels.hip): the QLoRA weight of torchao's NF4Tensor (quantization/quantize_/workflows/nf4/nf4_tensor.py) ----------------
// Every tensor is bf16; bf16(...) is an fp32 operation rounded ONCE to bf16, nearest even; divisions are correctly rounded fp32
// divisions; subnormals are kept.  A flattened tensor, blocks of B elements, scaler blocks of SB consecutive blocks:
//   cast (from_tensor :649-718; double_quantize_scalers :721-778; convert_to_norm_float_weight :806-843):
//     a[b]  = max |x| over block b (exact);   mean = bf16(mean of a) -- the only order-dependent value: torch computes it, the kernels
//     read it through a device pointer;   c[b] = bf16(a[b] - mean)
//     per scaler block:  m = max |c|;  qf = bf16(256 / bf16(2 m));  q[b] = int8(clamp(rint(bf16(c[b] qf)), -128, 127)), rint to even
//       -- m = 0: qf = inf, the product is NaN and the reference's NaN -> int8 is undefined; a NaN product writes 0 here
//     per element:  v = bf16(x / a[b]);  code = the FIRST i that minimises |bf16(v - table[i])| (quantize_tensor_nearest :874-880); a
//       NaN v (an all-zero block: 0 / 0) compares below nothing, code 0, as torch.min;  elements 2i | 2i + 1 share byte i, 2i in the
//       HIGH nibble
//   dequantize (get_original_weight :845-871; dequantize_scalers :780-803):
//     s[b] = bf16(bf16(f32(q[b]) / qf[b / SB]) + mean);   w = bf16(table[code] s[b]) (the product of two bf16 is exact in fp32)
//   linear (LinearNF4 :1053-1064):  y = bf16(sum_k x[m, k] w[n, k]), exact products, fp32 accumulation in any order
// The table (:666-684) rounded to bf16, as bits; every entry is a multiple of 2^-11.
__device__ __forceinline__ float nf4_value(uint32_t code) {
  constexpr uint32_t bits[16] = {0xbf800000u, 0xbf320000u, 0xbf060000u, 0xbeca0000u, 0xbe920000u, 0xbe3d0000u, 0xbdbb0000u, 0x00000000u,
                                 0x3da30000u, 0x3e250000u, 0x3e7c0000u, 0x3ead0000u, 0x3ee20000u, 0x3f100000u, 0x3f390000u, 0x3f800000u};
  return bits_to_f32(bits[code]);
}
// v (an fp32 holding a bf16) -> its code
__device__ __forceinline__ uint32_t nf4_code(float v) {
#pragma clang fp contract(off)
  uint32_t best = 0u;
  float bd = fabsf(round_bf16(v - nf4_value(0)));
#pragma unroll
  for (uint32_t i = 1; i < 16; ++i) {
    const float d = fabsf(round_bf16(v - nf4_value(i)));
    if (d < bd) {  // (false for a NaN: the first index stays)
      bd = d;
      best = i;
    }
  }
  return best;
}
// 8 bf16 of ONE block -> 8 codes, 4 bytes in memory order; a: the block's maximum
__device__ __forceinline__ uint32_t nf4_cast8(const u32x4& x, float a) {
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
  uint32_t o = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t hi = nf4_code(round_bf16(bf16_lo_to_f32(w[j]) / a)), lo = nf4_code(round_bf16(bf16_hi_to_f32(w[j]) / a));
    o |= ((hi << 4) | lo) << (8 * j);
  }
  return o;
}
// the centred scaler of a block and, from a scaler block's m, its quantization factor and a block's int8 scaler
__device__ __forceinline__ float nf4_centred(float a, float mean) { return round_bf16(a - mean); }
__device__ __forceinline__ float nf4_factor(float m) { return round_bf16(256.0f / round_bf16(2.0f * m)); }
__device__ __forceinline__ int nf4_scaler_q(float c, float qf) {
  const float p = round_bf16(mul_f32_rn(c, qf));
  return (p != p) ? 0 : (int)fminf(fmaxf(rintf(p), -128.f), 127.f);
}
// dequantize's scaler of a block: q its int8 scaler, qf the factor of its scaler block
__device__ __forceinline__ float nf4_scaler(int q, float qf, float mean) { return round_bf16(round_bf16((float)q / qf) + mean); }
// 8 codes (4 bytes in memory order) -> 8 bf16 = bf16(table[code] s); tab: the 16 fp32 table values in LDS
__device__ __forceinline__ u32x4 nf4_decode8(uint32_t c, float s, const float* tab) {
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(tab[(c >> (8 * j + 4)) & 15u] * s, tab[(c >> (8 * j)) & 15u] * s);
  return u32x4{o[0], o[1], o[2], o[3]};
}

// ---- low-bit optimizer states (optim_kernels.hip): torchao/optim's block-quantized Adam moments and its single_param_adam ----------------
// The reference's EAGER CPU run (adam.py:163-209 on the subclasses of subclass_8bit.py / subclass_4bit.py / subclass_fp8.py, helpers in
// quant_utils.py) is a fixed sequence of fp32 operations, each rounded ONCE; divisions and sqrt are correctly rounded; subnormals are kept;
// NaN and Inf are outside the contract.  A tensor is taken flat, in blocks of B elements (a power of two, 64 .. 2048):
//   tables     four qmaps (8-bit signed / unsigned dynamic maps of 256 entries, the 4-bit signed dynamic map and the 4-bit unsigned
//              linspace(0, 1, 17)[1:] of 16: no zero, a zero second moment decodes to scale / 16 -- the reference's behaviour, kept).  No kernel
//              holds a table: each reads the qmap field of the state it is given.
//   quantize   scale = max(amax |x|, 1e-12);  y = x / scale (a division, not a reciprocal multiply);  the branch-free descent
//              c += (y >= qmap[c + step]) ? step : 0 over step = 128 .. 1 (8 .. 1 for 4 bits);  then up = min(c + 1, last) and the code is up
//              iff y - qmap[c] >= (qmap[up] - qmap[c]) * 0.5 (ties go up);  4 bits: element 2i in the HIGH nibble of byte i (not NVFP4's order)
//   fp8        scale = max(amax |x|, 1e-12) / 448;  code = e4m3fn_rne(x / scale)
//   dequantize qmap[code] * scale;  fp8: f32(code) * scale
//   plain      (fewer than 4096 elements, or a count that B does not divide: moments in the parameter's dtype)  read: to fp32;  write: RNE
//   step       the host passes lr, lr wd, wd, 1 - b1, 1 - b2 (rounded from the Python doubles), bc1 = 1 - b1^t, sqrt(1 - b2^t), eps, computed
//              with the torch CPU operations the reference runs on its 0-dim tensors:
//                AdamW  p = p - (lr wd) p          Adam  g = g + wd p
//                m = lerp(m_old, g, 1 - b1);  v = lerp(v_old, g g, 1 - b2);  amsgrad: vmax = max(vmax_old, v), used below for v
//                denom = sqrt(v) / sqrt_bc2 + eps;  p = p - (lr (m / bc1)) / denom
//              m, v, vmax are quantized from the fp32 values the update used; p is stored RNE (or SR below)
//   lerp       ATen's CPU kernel: |w| < 0.5: fma(w, e - s, s), else fma(w - 1, e - s, e): ONE fused operation, an explicit fmaf here.  The
//              fixture maker (tests/golden/make_golden_optim.py) compares the reference's recording with the fused and the unfused form:
//              with betas (0.9, 0.999) the recorded bytes are the fused form's in every case and the unfused form misses some in each of
//              the 11 cases of 4096 elements or more; with (0.75, 0.9375) the product is exact and both agree.
//   sqrt       the IEEE one.  ATen's CPU sqrt of a contiguous tensor is MKL's vsSqrt, under an ulp but not correctly rounded (0.6% of
//              random inputs an ulp off; 7 recorded values of 3 fixture cases), on inputs that depend on the MKL build: the maker records
//              the reference with aten.sqrt taken through float64, and counts what MKL's root would have changed.
//   amsgrad    on a quantized state the reference's eager run raises (its subclasses implement no aten.maximum); the maker registers the
//              dequantizing form its lerp has, which is the line above.  On plain states the reference runs as it is.
//   SR         (bf16 p; the reference draws torch.randint, not reproducible here: this library's own contract)  away from zero iff
//              r16 < (bits & 0xFFFF): (bits & 0xFFFF0000) + 0x10000, else the truncation.  Philox4x32-10 (above), key = the halves of the
//              optimizer's int64 seed, counter = (g_lo, g_hi, step, param_index), g the flat index of the group of 8 consecutive elements;
//              element j takes bits 16 (j & 1) .. + 15 of output word j >> 1.  The bytes depend on (seed, step, param_index, element) only.
template <int BITS>
__device__ __forceinline__ uint32_t optim_table_code(float y, const float* tab) {
#pragma clang fp contract(off)
  uint32_t c = 0u;
#pragma unroll
  for (uint32_t step = 1u << (BITS - 1); step != 0u; step >>= 1) c += (y >= tab[c + step]) ? step : 0u;
  const uint32_t up = min(c + 1u, (1u << BITS) - 1u);
  const float dv = tab[c], uv = tab[up];
  return (y - dv >= (uv - dv) * 0.5f) ? up : c;
}
__device__ __forceinline__ float optim_block_scale(float amax) { return fmaxf(amax, 1e-12f); }
__device__ __forceinline__ float optim_fp8_scale(float amax) {
#pragma clang fp contract(off)
  return fmaxf(amax, 1e-12f) / 448.0f;
}
__device__ __forceinline__ float optim_lerp(float s, float e, float w) {
#pragma clang fp contract(off)
  const float d = e - s;
  return (fabsf(w) < 0.5f) ? __builtin_fmaf(w, d, s) : __builtin_fmaf(w - 1.0f, d, e);
}
// one element of the step: p, m, v, vmax in and out (fp32); returns nothing the states do not hold
__device__ __forceinline__ void optim_adam_element(float& p, float g, float& m, float& v, float& vmax, bool has_vmax, bool is_adamw,
                                                   const ao_optim_scalars& s) {
#pragma clang fp contract(off)
  if (is_adamw) {
    const float d = s.lr_wd * p;
    p = p - d;
  } else {
    const float d = s.wd * p;
    g = g + d;
  }
  m = optim_lerp(m, g, s.one_minus_beta1);
  const float g2 = g * g;
  v = optim_lerp(v, g2, s.one_minus_beta2);
  float den = v;
  if (has_vmax) {
    vmax = fmaxf(vmax, v);
    den = vmax;
  }
  const float denom = __builtin_sqrtf(den) / s.sqrt_bias_correction2 + s.eps;
  const float mh = m / s.bias_correction1;
  const float num = s.lr * mh;
  const float upd = num / denom;
  p = p - upd;
}
// fp32 -> bf16 bits under 16 random bits
__device__ __forceinline__ uint32_t optim_sr_bf16(float x, uint32_t r16) {
  const uint32_t b = f32_to_bits(x);
  return ((b & 0xffff0000u) + ((r16 < (b & 0xffffu)) ? 0x10000u : 0u)) >> 16;
}

// ---- the int4 group recipe (mslk's int4_row_quantize_zp / int4_row_quantize as the reference restates them: qat/fake_quantizer.py:148-190,
// prototype/gptq/api.py:167-221), in fp32, every step ONE operation rounded once, the divisions IEEE.  Over a group of g elements along K:
//   asymmetric:  s = max(max - min, 1e-6) / 15;  z = min + 8 s;  q = clamp(rint((w - min) / s), 0, 15)      (stored as q - 8)
//   symmetric:   s = max(max|w| / 8, 1e-6);      z = 0;          q = clamp(rint(w / s), -8, 7)
// The ONE definition: ao_int4_plain_quantize (what `convert` stores), the QAT fake quantizer and its backward, the AWQ search and GPTQ's
// qparams all come here, so "the codes are those of ao_int4_plain_quantize" is a statement about these lines.  What a caller does with a
// code -- (q - 8) s + z in fp32, the stored weight through bf16(s) and bf16(z), GPTQ's own m = z - 8 s -- is that caller's arithmetic.
__device__ __forceinline__ void int4_group_qparams(float mx, float mn, float& s, float& z) {
#pragma clang fp contract(off)
  s = fmaxf(mx - mn, 1e-6f) / 15.0f;
  z = mn + s * 8.0f;  // (8 s is exact: contracted or not, one rounding)
}
__device__ __forceinline__ float int4_group_scale_sym(float amax) { return fmaxf(amax / 8.0f, 1e-6f); }
// the unsigned code 0 .. 15 of x in a group of minimum m and scale s
__device__ __forceinline__ float int4_group_code(float x, float m, float s) {
#pragma clang fp contract(off)
  return fminf(fmaxf(rintf((x - m) / s), 0.f), 15.f);
}

// ---- a tensor as a flat run of 16-byte vectors of 8 bf16, one per lane; a group is LANES = g / 8 adjacent lanes (K % g == 0 keeps groups
// whole inside a row, and LANES divides the wave), so every group reduction is a butterfly over lanes: no LDS, no atomics -----------------
__device__ __forceinline__ void unpack_bf16x8(const u32x4& v, float (&f)[8]) {
  f[0] = bf16_lo_to_f32(v.x), f[1] = bf16_hi_to_f32(v.x), f[2] = bf16_lo_to_f32(v.y), f[3] = bf16_hi_to_f32(v.y);
  f[4] = bf16_lo_to_f32(v.z), f[5] = bf16_hi_to_f32(v.z), f[6] = bf16_lo_to_f32(v.w), f[7] = bf16_hi_to_f32(v.w);
}
__device__ __forceinline__ u32x4 pack_bf16x8(const float (&f)[8]) {
  return u32x4{pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
}
template <int LANES>
__device__ __forceinline__ void group_range(const float (&x)[8], float& mx, float& mn) {
  mx = x[0], mn = x[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) {
    mx = fmaxf(mx, x[j]);
    mn = fminf(mn, x[j]);
  }
#pragma unroll
  for (int off = 1; off < LANES; off <<= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, off));
    mn = fminf(mn, __shfl_xor(mn, off));
  }
}
// every lane of the group ends with the same bits: a + b and b + a round alike
template <int LANES>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = 1; off < LANES; off <<= 1) v += __shfl_xor(v, off);
  return v;
}

}  // namespace ao
