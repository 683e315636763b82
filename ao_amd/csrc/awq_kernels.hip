// AWQ scale search for gfx950: the error matrices of R candidate scale vectors in ONE launch that reads the weight once.
//
// Reference (torchao 0.19.0 snapshot): prototype/awq/core.py:70-86.  For each of its 20 ratios the reference scales the weight, runs the whole
// int4 quantize_ handler on it and compares two F.linear outputs over every calibration token.  The loss it minimises,
// mean((X W^T - (X / s) Wq^T)^2), is tr(D G D^T) / (rows N) with D = W - Wq / s and G = X^T X, so what the search needs of the weight is D.
// Per ratio r, row n and group of g columns, every step ONE fp32 operation rounded once (IEEE division, no fma contraction):
//   ws  = bf16(f32(W[n,k]) * f32(S[r,k]))                          core.py:78 `self.weight * scales`, a bf16 tensor op
//   M, m = max, min of ws over the group;  s = max(M - m, 1e-6) / 15;  z = m + 8 s       int4_group_qparams (quant_math.h)
//   q   = clamp(rint((ws - m) / s), 0, 15) - 8                      int4_group_code: the codes of ao_int4_plain_quantize
//   dq  = bf16(f32(bf16(q * f32(bf16(s)))) + f32(bf16(z)))          the weight int4_plain_kernels.hip's header states: the qparams are STORED
//                                                                   as bf16, and the product and the sum are bf16 tensor ops
//   D[r,n,k] = f32(W[n,k]) - f32(dq) / f32(S[r,k])                  the division, then the subtraction
// so dq is Int4Tensor.from_hp(W * S[r], [1, g]).dequantize() byte for byte: the codes `convert` will store are the codes the search judged.
// (q * bf16(s) has 4 x 8 significand bits and W * S 8 x 8: both products are exact in fp32, their one rounding is the one to bf16.)
//
// Structure: the weight is a flat run of 16-byte vectors, one per lane (quant_math.h's lane helpers, shared with the fake quantizer); a group is
// g / 8 adjacent lanes (K % g == 0 keeps groups whole inside a row) and its range a butterfly over lanes: no LDS, no atomics, the same bytes
// every launch.  The lane keeps its 8 weights in registers and loops over r; row r of S is read as one 16-byte piece per lane (R K bf16, it
// stays in L2) and D is written as two 16-byte stores per lane that together fill whole 32-byte runs.  The loop is unrolled by two, so that
// the next row of S is in flight during the divisions of this one; 40 - 43 VGPRs, no scratch, 8 waves a SIMD.  Measured:
// 2.4 - 3.3 TB/s of its (2 + 4 R) bytes an element on the Llama-3-8B shapes, 1 - 2 % of a search, whose time is the host's fp32 matmul.
//
// The lane helpers (unpack_bf16x8, group_range) and the recipe (int4_group_qparams, int4_group_code) are quant_math.h's, the lines
// ao_int4_plain_quantize runs.  The fake quantizer's int4_fq_value is not used: it is (q - 8) s + z with fp32 qparams, one rounding fewer
// than the stored weight above.
#include "common.h"
#include "quant_math.h"

namespace ao {
namespace {

constexpr int kThreads = 256;

// one element's D from its weight w, its scaled weight ws, its candidate scale sc and the group's m, s, bf16(s), bf16(z)
__device__ __forceinline__ float awq_error_value(float w, float ws, float sc, float m, float s, float sb, float zb) {
#pragma clang fp contract(off)
  const float q = int4_group_code(ws, m, s) - 8.f;
  const float p = round_bf16(q * sb);
  const float dq = round_bf16(p + zb);
  const float back = dq / sc;
  return w - back;
}

template <int G>
__global__ __launch_bounds__(kThreads) void awq_scaled_error_kernel(const u32x4* __restrict__ w, const u32x4* __restrict__ scales,
                                                                     f32x4* __restrict__ d, int64_t nvec, int64_t kvec, int R) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < nvec;  // (a group is live or dead as a whole; dead lanes still take part in the butterflies, on in-bounds reads)
  const u32x4 raw = live ? w[i] : u32x4{0u, 0u, 0u, 0u};
  const u32x4* srow = scales + (live ? i % kvec : 0);
  f32x4* drow = d + 2 * i;
  float x[8];
  unpack_bf16x8(raw, x);
#pragma unroll 2
  for (int r = 0; r < R; ++r) {
    float sc[8], ws[8], M, m, s, z;
    unpack_bf16x8(srow[(int64_t)r * kvec], sc);
#pragma unroll
    for (int j = 0; j < 8; ++j) ws[j] = round_bf16(x[j] * sc[j]);
    group_range<G / 8>(ws, M, m);
    int4_group_qparams(M, m, s, z);
    const float sb = round_bf16(s), zb = round_bf16(z);
#pragma unroll
    for (int j = 0; j < 8; ++j) ws[j] = awq_error_value(x[j], ws[j], sc[j], m, s, sb, zb);
    if (live) {
      f32x4* out = drow + (int64_t)r * (2 * nvec);
      out[0] = f32x4{ws[0], ws[1], ws[2], ws[3]};
      out[1] = f32x4{ws[4], ws[5], ws[6], ws[7]};
    }
  }
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_awq_scaled_error(const uint16_t* w, const uint16_t* scales, float* d, int64_t N, int64_t K, int64_t R, int group_size,
                                   void* stream) {
  AO_REQUIRE(N >= 0 && R >= 0 && K > 0, "%s: bad shape N=%lld K=%lld R=%lld", __func__, (long long)N, (long long)K, (long long)R);
  AO_REQUIRE(group_size == 32 || group_size == 64 || group_size == 128 || group_size == 256,
             "%s: group_size must be one of 32, 64, 128, 256, got %d", __func__, group_size);
  AO_REQUIRE(K % group_size == 0, "%s: K=%lld must be a multiple of group_size=%d", __func__, (long long)K, group_size);
  AO_REQUIRE(R < (1ll << 31) && N <= (1ll << 60) / K && (R == 0 || N * K <= (1ll << 60) / R) &&
                 (N * K / 8 + kThreads - 1) / kThreads < (1ll << 31),
             "%s: N=%lld K=%lld R=%lld too large for one launch", __func__, (long long)N, (long long)K, (long long)R);
  if (N == 0 || R == 0) return AO_OK;
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(scales);
  AO_REQUIRE_PTR(d);
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(scales, 16) && aligned_to(d, 16), "%s: w, scales and d must be 16-byte aligned", __func__);
  hipStream_t st = (hipStream_t)stream;
  const int64_t nvec = N * K / 8, kvec = K / 8;
  const dim3 grid((unsigned)((nvec + kThreads - 1) / kThreads)), block(kThreads);
  const u32x4* wv = reinterpret_cast<const u32x4*>(w);
  const u32x4* sv = reinterpret_cast<const u32x4*>(scales);
  f32x4* dv = reinterpret_cast<f32x4*>(d);
  with_group_size(group_size, [&](auto g) {
    ao::launch(awq_scaled_error_kernel<decltype(g)::value>, grid, block, 0, st, wv, sv, dv, nvec, kvec, (int)R);
  });
  AO_LAUNCH_CHECK("awq_scaled_error_kernel launch");
  return AO_OK;
}
