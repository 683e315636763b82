// Quantization-aware training for gfx950: the fake quantizers of torchao.quantization.qat as ONE launch per direction, bf16 -> bf16.
//
// Reference (torchao 0.19.0 snapshot):
//   int4 : qat/fake_quantizer.py:167-187 (Int4WeightFakeQuantizer._bf16_activations_forward), in fp32, per group of g along K:
//            M = max, m = min;  s = max(M - m, 1e-6) / 15;  z = m + 8 s
//            q = clamp(rint((w - m) / s), 0, 15);  out = bf16((q - 8) s + z)        (two roundings: the product, then the sum)
//          s, z and q are int4_group_qparams and int4_group_code (quant_math.h), the lines ao_int4_plain_quantize runs: the codes are the
//          ones `convert` stores.
//   fp8  : qat/fake_quantizer.py:84-98 (Float8FakeQuantizer.forward, PerRow, e4m3) over quant_primitives.py:2173-2304, per row:
//            a = clamp(max|x|, lb, ub)                     in the INPUT's dtype: bf16, so lb and ub take effect as bf16 values
//            s = f32(bf16(a / 448))                        (_choose_scale_float8 divides the bf16 amax: the scale is a bf16 value)
//            t = f32(x) / s;  q = e4m3_rne(clamp(t, -448, 448));  out = bf16(f32(q) s)
//          An all-zero row without a lower bound has s = 0 and t = 0 / 0: the reference's row is NaN, and so is this one.
// Every `/` is the correctly rounded fp32 division (hipcc's default), like torch's.
//
// Backward: only the input is saved; M, m, s, q are made again from it and no mask is stored.  G = f32(grad_out), t the unclamped
// quotient, c = 1 where the clamp passes its gradient (inclusive at both ends, like torch's clamp backward), d = q - c t:
//   int4 : ds = sum G d;  dm = sum G (1 - c);  dr = ds / 15 where M - m >= 1e-6, else 0
//          grad_w = G c + [w = M] dr / #{w = M} + [w = m] (dm - dr) / #{w = m}          -- the reference's own autograd
//   fp8  : ds = sum G d;  da = ds / 448 where lb <= max|x| <= ub, else 0
//          grad_x = G c + [|x| = max|x|] sign(x) da / #{|x| = max|x|}                    -- the chain with every cast straight-through
//          (the reference's autograd rounds the incoming gradient to e4m3 at `.to(float32)` of the fp8 tensor: DESIGN.md 4.24)
// d is summed as one term: q and c t are each as large as the clamp bound and nearly cancel, their difference is the rounding residue.
// Ties share the range term evenly (amax / amin in autograd).  Sums are fp32, in a fixed order: no atomics, the same bytes every launch.
#include "common.h"
#include "quant_math.h"

namespace ao {
namespace {

constexpr int kThreads = kRowThreads;

// ---- int4: the tensor as a flat run of 16-byte vectors, one per lane; a group is G / 8 adjacent lanes.  The lane helpers (unpack_bf16x8,
// group_range, group_sum) and the recipe (int4_group_qparams, int4_group_code) are quant_math.h's -------------------------------------------

// (q - 8) s + z as the reference's two tensor ops: the product rounded, then the sum
__device__ __forceinline__ float int4_fq_value(float x, float m, float s, float z) {
#pragma clang fp contract(off)
  const float p = (int4_group_code(x, m, s) - 8.f) * s;
  return p + z;
}

template <int G>
__global__ __launch_bounds__(kThreads) void qat_int4_fake_quantize_kernel(const u32x4* __restrict__ w, u32x4* __restrict__ out,
                                                                           int64_t nvec) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < nvec;  // (a group is live or dead as a whole; dead lanes still take part in the butterflies)
  const u32x4 raw = live ? w[i] : u32x4{0u, 0u, 0u, 0u};
  float x[8], M, m, s, z;
  unpack_bf16x8(raw, x);
  group_range<G / 8>(x, M, m);
  int4_group_qparams(M, m, s, z);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = int4_fq_value(x[j], m, s, z);
  if (live) out[i] = pack_bf16x8(x);
}

template <int G>
__global__ __launch_bounds__(kThreads) void qat_int4_fake_quantize_bwd_kernel(const u32x4* __restrict__ w, const u32x4* __restrict__ go,
                                                                               u32x4* __restrict__ gw, int64_t nvec) {
  constexpr int LANES = G / 8;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < nvec;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const u32x4 raw = live ? w[i] : zero4, graw = live ? go[i] : zero4;
  float x[8], g[8], M, m, s, z;
  unpack_bf16x8(raw, x);
  unpack_bf16x8(graw, g);
  group_range<LANES>(x, M, m);
  int4_group_qparams(M, m, s, z);  // (z is not used: only the scale and the codes enter the gradient)
  float ds = 0.f, dm = 0.f, n_max = 0.f, n_min = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t = (x[j] - m) / s, r = rintf(t);
    const bool inside = r >= 0.f && r <= 15.f;
    const float q = int4_group_code(x[j], m, s);  // (= clamp(r, 0, 15): the same quotient)
    ds += g[j] * (inside ? q - t : q);
    dm += inside ? 0.f : g[j];
    n_max += x[j] == M ? 1.f : 0.f;
    n_min += x[j] == m ? 1.f : 0.f;
    g[j] = inside ? g[j] : 0.f;  // G c
  }
  ds = group_sum<LANES>(ds);
  dm = group_sum<LANES>(dm);
  n_max = group_sum<LANES>(n_max);
  n_min = group_sum<LANES>(n_min);
  const float dr = (M - m >= 1e-6f) ? ds / 15.0f : 0.f;
  const float to_max = dr / n_max, to_min = (dm - dr) / n_min;
#pragma unroll
  for (int j = 0; j < 8; ++j) g[j] += (x[j] == M ? to_max : 0.f) + (x[j] == m ? to_min : 0.f);
  if (live) gw[i] = pack_bf16x8(g);
}

// ---- fp8: a workgroup owns a row.  NV = 16-byte vectors a thread holds (the row stays in registers between the amax and the second
// use); NV = 0 walks the row again, out of L2.  block_max / block_sum: common.h ----------------------------------------------------------------
__device__ __forceinline__ float vec_amax(const u32x4& v) {
  bool has_nan = false;  // (non-finite inputs are outside the contract; amax8 asks for the flag)
  return amax8(v, has_nan);
}

// the clamped amax and the scale; lb / ub act as the bf16 values torch.clamp makes of them on a bf16 tensor
__device__ __forceinline__ float qat_fp8_scale(float amax, float lb, float ub, bool& amax_inside) {
  lb = round_bf16(lb), ub = round_bf16(ub);
  amax_inside = amax >= lb && amax <= ub;
  return round_bf16(fminf(fmaxf(amax, lb), ub) / 448.0f);
}

// four quotients -> their e4m3 codes -> fp32 again
__device__ __forceinline__ void e4m3_round4(const float* t, float* q) {
  const uint32_t codes = cvt4_e4m3(clamp448(t[0]), clamp448(t[1]), clamp448(t[2]), clamp448(t[3]));
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)codes, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)codes, true);
  q[0] = lo.x, q[1] = lo.y, q[2] = hi.x, q[3] = hi.y;
}

// A NaN leaves as 0xFFFF, the pattern the reference's CPU chain ends in (its 0 / 0 is x86's negative quiet NaN, which e4m3 keeps as byte
// 0xFF): an all-zero row without a lower bound is that row, bit for bit.
__device__ __forceinline__ uint32_t fq_bf16_bits(float v) { return (v != v) ? 0xffffu : (uint32_t)f32_to_bf16_bits(v); }

__device__ __forceinline__ u32x4 fp8_fq8(const u32x4& v, float s) {
  float x[8], q[8];
  unpack_bf16x8(v, x);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = x[j] / s;
  e4m3_round4(x, q);
  e4m3_round4(x + 4, q + 4);
  uint32_t o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = fq_bf16_bits(q[j] * s);
  return u32x4{o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16)};
}

template <int NV>
__global__ __launch_bounds__(kThreads) void qat_fp8_fake_quantize_rowwise_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ out,
                                                                                  int64_t C, float lb, float ub) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x, nvec = C >> 3;
  const u32x4* xr = reinterpret_cast<const u32x4*>(x + row * C);
  u32x4* orow = reinterpret_cast<u32x4*>(out + row * C);
  constexpr int NR = NV > 0 ? NV : 1;
  u32x4 v[NR];
  float m = 0.f;
  if (NV > 0) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int64_t idx = threadIdx.x + i * kThreads;
      v[i] = (idx < nvec) ? xr[idx] : u32x4{0u, 0u, 0u, 0u};
      m = fmaxf(m, vec_amax(v[i]));
    }
  } else {
    for (int64_t i = threadIdx.x; i < nvec; i += kThreads) m = fmaxf(m, vec_amax(xr[i]));
  }
  m = block_max(m, red);
  bool amax_inside;
  const float s = qat_fp8_scale(m, lb, ub, amax_inside);
  if (NV > 0) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int64_t idx = threadIdx.x + i * kThreads;
      if (idx < nvec) orow[idx] = fp8_fq8(v[i], s);
    }
  } else {
    for (int64_t i = threadIdx.x; i < nvec; i += kThreads) orow[i] = fp8_fq8(xr[i], s);
  }
}

// one vector's share of ds = sum G (q - c t) and of #{|x| = amax}; G c is left in g
__device__ __forceinline__ void fp8_bwd_terms(const u32x4& xv, const u32x4& gv, float s, float amax, float (&x)[8], float (&g)[8], float& ds,
                                              float& n_max) {
  float t[8], q[8];
  unpack_bf16x8(xv, x);
  unpack_bf16x8(gv, g);
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = x[j] / s;
  e4m3_round4(t, q);
  e4m3_round4(t + 4, q + 4);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool inside = t[j] >= -448.f && t[j] <= 448.f;
    ds += g[j] * (inside ? q[j] - t[j] : q[j]);
    n_max += fabsf(x[j]) == amax ? 1.f : 0.f;
    g[j] = inside ? g[j] : 0.f;
  }
}
__device__ __forceinline__ u32x4 fp8_bwd_grad8(const float (&x)[8], const float (&g)[8], float amax, float share) {
  uint32_t o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float sign = x[j] > 0.f ? 1.f : (x[j] < 0.f ? -1.f : 0.f);
    o[j] = fq_bf16_bits(g[j] + (fabsf(x[j]) == amax ? sign * share : 0.f));
  }
  return u32x4{o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16)};
}

template <int NV>
__global__ __launch_bounds__(kThreads) void qat_fp8_fake_quantize_rowwise_bwd_kernel(const uint16_t* __restrict__ x,
                                                                                      const uint16_t* __restrict__ go,
                                                                                      uint16_t* __restrict__ gx, int64_t C, float lb,
                                                                                      float ub) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x, nvec = C >> 3;
  const u32x4* xr = reinterpret_cast<const u32x4*>(x + row * C);
  const u32x4* gr = reinterpret_cast<const u32x4*>(go + row * C);
  u32x4* orow = reinterpret_cast<u32x4*>(gx + row * C);
  constexpr int NR = NV > 0 ? NV : 1;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  u32x4 v[NR], gv[NR];
  float m = 0.f;
  if (NV > 0) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int64_t idx = threadIdx.x + i * kThreads;
      v[i] = (idx < nvec) ? xr[idx] : zero4;
      gv[i] = (idx < nvec) ? gr[idx] : zero4;  // (asked for before the amax meets: in flight during it)
      m = fmaxf(m, vec_amax(v[i]));
    }
  } else {
    for (int64_t i = threadIdx.x; i < nvec; i += kThreads) m = fmaxf(m, vec_amax(xr[i]));
  }
  m = block_max(m, red);
  bool amax_inside;
  const float s = qat_fp8_scale(m, lb, ub, amax_inside);
  float ds = 0.f, n_max = 0.f;
  float xf[NR][8], gc[NR][8];
  if (NV > 0) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int64_t idx = threadIdx.x + i * kThreads;
      if (idx < nvec) fp8_bwd_terms(v[i], gv[i], s, m, xf[i], gc[i], ds, n_max);
    }
  } else {
    for (int64_t i = threadIdx.x; i < nvec; i += kThreads) fp8_bwd_terms(xr[i], gr[i], s, m, xf[0], gc[0], ds, n_max);
  }
  ds = block_sum(ds, red);
  n_max = block_sum(n_max, red);
  const float share = (amax_inside ? ds / 448.0f : 0.f) / n_max;
  if (NV > 0) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int64_t idx = threadIdx.x + i * kThreads;
      if (idx < nvec) orow[idx] = fp8_bwd_grad8(xf[i], gc[i], m, share);
    }
  } else {
    for (int64_t i = threadIdx.x; i < nvec; i += kThreads) {
      float ds2 = 0.f, n2 = 0.f;
      fp8_bwd_terms(xr[i], gr[i], s, m, xf[0], gc[0], ds2, n2);
      orow[i] = fp8_bwd_grad8(xf[0], gc[0], m, share);
    }
  }
}

int check_int4(const char* fn, int64_t N, int64_t K, int g) {
  AO_REQUIRE(N >= 0 && K > 0, "%s: bad shape N=%lld K=%lld", fn, (long long)N, (long long)K);
  AO_REQUIRE(g == 32 || g == 64 || g == 128 || g == 256, "%s: group_size must be one of 32, 64, 128, 256, got %d", fn, g);
  AO_REQUIRE(K % g == 0, "%s: K=%lld must be a multiple of group_size=%d", fn, (long long)K, g);
  AO_REQUIRE(N <= (1ll << 62) / K && (N * K / 8 + kThreads - 1) / kThreads < (1ll << 31), "%s: N=%lld K=%lld too large for one launch", fn,
             (long long)N, (long long)K);
  return AO_OK;
}

int check_fp8(const char* fn, int64_t R, int64_t C, float lb, float ub) {
  AO_REQUIRE(R >= 0 && C > 0, "%s: bad shape R=%lld C=%lld", fn, (long long)R, (long long)C);
  AO_REQUIRE(C % 16 == 0, "%s: C=%lld must be a multiple of 16", fn, (long long)C);
  AO_REQUIRE(R < (1ll << 31), "%s: R=%lld too large for one launch", fn, (long long)R);
  AO_REQUIRE(lb <= ub, "%s: hp_value_lb=%g must not exceed hp_value_ub=%g (pass -inf / +inf for an absent bound)", fn, (double)lb, (double)ub);
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_qat_int4_fake_quantize(const uint16_t* w, uint16_t* out, int64_t N, int64_t K, int group_size, void* stream) {
  if (int rc = check_int4(__func__, N, K, group_size)) return rc;
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(out, 16), "%s: w and out must be 16-byte aligned", __func__);
  hipStream_t st = (hipStream_t)stream;
  const int64_t nvec = N * K / 8;
  const dim3 grid((unsigned)((nvec + kThreads - 1) / kThreads)), block(kThreads);
  with_group_size(group_size, [&](auto g) {
    ao::launch(qat_int4_fake_quantize_kernel<decltype(g)::value>, grid, block, 0, st, reinterpret_cast<const u32x4*>(w),
               reinterpret_cast<u32x4*>(out), nvec);
  });
  AO_LAUNCH_CHECK("qat_int4_fake_quantize_kernel launch");
  return AO_OK;
}

extern "C" int ao_qat_int4_fake_quantize_bwd(const uint16_t* w, const uint16_t* grad_out, uint16_t* grad_w, int64_t N, int64_t K,
                                             int group_size, void* stream) {
  if (int rc = check_int4(__func__, N, K, group_size)) return rc;
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(grad_out);
  AO_REQUIRE_PTR(grad_w);
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(grad_out, 16) && aligned_to(grad_w, 16), "%s: w, grad_out and grad_w must be 16-byte aligned",
             __func__);
  hipStream_t st = (hipStream_t)stream;
  const int64_t nvec = N * K / 8;
  const dim3 grid((unsigned)((nvec + kThreads - 1) / kThreads)), block(kThreads);
  with_group_size(group_size, [&](auto g) {
    ao::launch(qat_int4_fake_quantize_bwd_kernel<decltype(g)::value>, grid, block, 0, st, reinterpret_cast<const u32x4*>(w),
               reinterpret_cast<const u32x4*>(grad_out), reinterpret_cast<u32x4*>(grad_w), nvec);
  });
  AO_LAUNCH_CHECK("qat_int4_fake_quantize_bwd_kernel launch");
  return AO_OK;
}

extern "C" int ao_qat_fp8_fake_quantize_rowwise(const uint16_t* x, uint16_t* out, int64_t R, int64_t C, float lb, float ub, void* stream) {
  if (int rc = check_fp8(__func__, R, C, lb, ub)) return rc;
  if (R == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(out, 16), "%s: x and out must be 16-byte aligned", __func__);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)R), block(kThreads);
  auto go = [&](auto nv) { ao::launch(qat_fp8_fake_quantize_rowwise_kernel<decltype(nv)::value>, grid, block, 0, st, x, out, C, lb, ub); };
  if (!with_row_depth(C, go)) go(std::integral_constant<int, 0>{});  // longer rows: the walking form
  AO_LAUNCH_CHECK("qat_fp8_fake_quantize_rowwise_kernel launch");
  return AO_OK;
}

extern "C" int ao_qat_fp8_fake_quantize_rowwise_bwd(const uint16_t* x, const uint16_t* grad_out, uint16_t* grad_x, int64_t R, int64_t C,
                                                    float lb, float ub, void* stream) {
  if (int rc = check_fp8(__func__, R, C, lb, ub)) return rc;
  if (R == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(grad_out);
  AO_REQUIRE_PTR(grad_x);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(grad_out, 16) && aligned_to(grad_x, 16), "%s: x, grad_out and grad_x must be 16-byte aligned",
             __func__);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)R), block(kThreads);
  auto go = [&](auto nv) {
    ao::launch(qat_fp8_fake_quantize_rowwise_bwd_kernel<decltype(nv)::value>, grid, block, 0, st, x, grad_out, grad_x, C, lb, ub);
  };
  if (!with_row_depth(C, go)) go(std::integral_constant<int, 0>{});
  AO_LAUNCH_CHECK("qat_fp8_fake_quantize_rowwise_bwd_kernel launch");
  return AO_OK;
}
