// Dynamic-activation 8-bit linears at decode sizes with the activation cast FUSED into the matmul:
//
//   int8:  xq, sx = per-row symmetric int8 of x;  y = bf16(bf16(i32(xq . wq^T) * sx[m]) * sw[n] + bias[n])
//          (Int8Tensor F.linear with act_quant_kwargs: int8_tensor.py:176-248 + :305-359)
//   fp8 :  xq, sx = per-row e4m3 of x;            y = bf16((xq . wq^T) * sx[m] * sw[n] + bias[n])
//          (Float8Tensor F.linear with act_quant_kwargs: float8_tensor.py:167-253 + float8/inference.py:104-123)
//
// One launch instead of two (the stand-alone cast costs 2.7-5 us per linear at M = 1, as much as a small projection).
// Structure = the per-tile weight-streaming kernel (stream8_kernels.hip): one workgroup per 16-wide n-tile, waves split
// K, weights straight into VGPRs.  Every workgroup first casts the whole activation itself -- M x K bf16 from L2, at
// most 64 KiB of codes -- into LDS with exactly the arithmetic of the stand-alone kernels (quant_math.h), then feeds
// its MFMAs from there; rows are K + 16 bytes apart so that the 16-byte operand reads of different rows hit different
// banks.  Same bits as cast + matmul (int8 bit-exact end to end).
#include "common.h"
#include "gemm8_route.h"
#include "quant_math.h"
#include "stream_blocks.h"

#include <algorithm>

namespace ao {
// dec8_kernels.hip (round 4): the same linear with the weights as full lines in a register ring and the cast under their flight
int dec8_dynamic(bool int8, const uint16_t* x, const void* wq, const float* w_scale, const uint16_t* bias, uint16_t* y, int64_t M, int64_t N,
                 int64_t K, const Dec8Shape& s, hipStream_t stream);
// mid8_kernels.hip (round 4): 16 < M <= 256 with few output tiles -- the per-row cast shared out among the workgroups of the same launch
int mid8_dynamic(bool int8, const uint16_t* x, const void* b, const float* scale_b, const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                 const Mid8Plan& plan, hipStream_t stream);
namespace {

struct Dyn8Args {
  const uint16_t* x;       // [M][K] bf16
  const uint8_t* b;        // [N][K] int8 / e4m3
  const float* col_scale;  // [N]
  const uint16_t* bias;    // [N] bf16 or null
  uint16_t* out;           // [M][N] bf16
  int M, N, K;
};

constexpr int kMaxRows = 16;

template <bool INT8>
__global__ __launch_bounds__(512) void dyn8_kernel(Dyn8Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = blockDim.x >> 6;
  const int stride = p.K + 16;                                       // bytes between rows of codes
  char* xq = smem;                                                   // [M][K + 16]
  float* wmax = reinterpret_cast<float*>(smem + p.M * stride);       // [nwaves][16] per-wave row maxima
  float* rs = wmax + nwaves * kMaxRows;                              // [16] row scales
  float* red = rs + kMaxRows;                                        // [nwaves][256] split-K partials

  // ---- 1. + 2. per-row amax -> scale, then the cast into LDS (every workgroup, redundantly: the activation is L2-resident and tiny)
  cast_rows_to_lds<INT8, false>(p.x, p.M, p.K, xq, stride, wmax, rs);
  __syncthreads();

  // ---- 3. stream this n-tile's weights past the codes
  const int ntile = blockIdx.x;
  const int ksteps = p.K >> 7;  // 128 k per step
  const int ks0 = (ksteps * wave) / nwaves, ks1 = (ksteps * (wave + 1)) / nwaves;
  const int n = ntile * 16 + (lane & 15);
  const int kq = lane >> 4;
  // operand layout of the K = 128 step (stream8_kernels.hip): lane group kq holds k = 16 kq .. +15 and 64 + 16 kq .. +15
  const uint8_t* brow = p.b + (size_t)n * p.K + kq * 16;
  const bool valid = (lane & 15) < p.M;
  const char* arow = xq + (valid ? (lane & 15) : 0) * stride + kq * 16;  // rows past M read row 0 (broadcast) and are zeroed
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};  // int8: int32 bit patterns
  for (int ks = ks0; ks < ks1; ++ks) {
    const u32x4 b0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(brow + (size_t)ks * 128));
    const u32x4 b1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(brow + (size_t)ks * 128 + 64));
    u32x4 a0 = *reinterpret_cast<const u32x4*>(arow + ks * 128);
    u32x4 a1 = *reinterpret_cast<const u32x4*>(arow + ks * 128 + 64);
    if (!valid) { a0 = u32x4{0, 0, 0, 0}; a1 = u32x4{0, 0, 0, 0}; }
    acc = mfma8_k128<INT8>(a0, a1, b0, b1, acc);
  }

  // ---- 4. split-K reduction across waves (wave order: reproducible), scales, store
  park_tile(red + (size_t)wave * 256, kq, lane & 15, acc);
  __syncthreads();
  for (int idx = threadIdx.x; idx < 256; idx += blockDim.x) {
    const int row = idx >> 4, col = idx & 15;
    if (row >= p.M) continue;
    const int gn = ntile * 16 + col;
    float c;
    if constexpr (INT8) {
      int isum = 0;
      for (int w = 0; w < nwaves; ++w) isum += __float_as_int(red[(size_t)w * 256 + idx]);
      c = (float)isum;
    } else {
      c = 0.f;
      for (int w = 0; w < nwaves; ++w) c += red[(size_t)w * 256 + idx];
    }
    float v = epilogue8<INT8>(c, rs[row], p.col_scale[gn]);
    if (p.bias != nullptr) v += bf16_lo_to_f32(p.bias[gn]);
    p.out[(size_t)row * p.N + gn] = f32_to_bf16_bits(v);
  }
}

template <bool INT8>
int launch_dyn8(const Dyn8Args& p, hipStream_t stream) {
  const int ksteps = p.K >> 7;
  int wpb = 1;
  while (wpb < 8 && ksteps / (wpb * 2) >= 2) wpb *= 2;
  const size_t smem = (size_t)p.M * (p.K + 16) + (size_t)(wpb * kMaxRows + kMaxRows + wpb * 256) * sizeof(float);
  auto kern = dyn8_kernel<INT8>;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), smem, "hipFuncSetAttribute(dyn8_kernel)")) return rc;
  ao::launch(kern, dim3((unsigned)(p.N / 16)), dim3(wpb * 64), smem, stream, p);
  AO_LAUNCH_CHECK("dyn8_kernel launch");
  return AO_OK;
}

// validates the shape and routes it once (*r: the route of the calling thread's overrides)
int check_dyn(const char* fn, bool int8, int64_t M, int64_t N, int64_t K, Gemm8Route* r) {
  AO_REQUIRE(M >= 0 && N > 0 && K > 0, "%s: bad shape M=%lld N=%lld K=%lld", fn, (long long)M, (long long)N, (long long)K);
  AO_REQUIRE(N % 16 == 0 && K % 128 == 0, "%s: N=%lld must be a multiple of 16 and K=%lld of 128", fn, (long long)N, (long long)K);
  *r = gemm8_route(int8 ? Gemm8Entry::Int8Dyn : Gemm8Entry::Fp8Dyn, M, N, K, true, gemm8_force());
  AO_REQUIRE(M == 0 || r->kernel != Gemm8Kernel::Invalid,
             "%s: the fused form holds the cast activation in LDS: M <= 16 and M * (K + 16) <= 65536 (or 16 < M <= 256 on a weight with "
             "few output tiles and K %% 512 == 0), got M=%lld K=%lld (use the cast + matmul entry points)", fn, (long long)M, (long long)K);
  AO_REQUIRE(N < (1ll << 31) && K < (1ll << 31), "%s: dimension too large", fn);
  return AO_OK;
}

template <bool INT8>
int dyn_linear(const Gemm8Route& r, const uint16_t* x, const uint8_t* wq, const float* w_scale, const uint16_t* bias, uint16_t* y, int64_t M,
               int64_t N, int64_t K, hipStream_t stream) {
  if (r.kernel == Gemm8Kernel::Mid8) return mid8_dynamic(INT8, x, wq, w_scale, bias, y, M, N, K, r.mid, stream);
  if (r.kernel == Gemm8Kernel::Dec8) return dec8_dynamic(INT8, x, wq, w_scale, bias, y, M, N, K, r.dec, stream);
  Dyn8Args p{x, wq, w_scale, bias, y, (int)M, (int)N, (int)K};
  return launch_dyn8<INT8>(p, stream);
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_dyn_linear_fits(int64_t M, int64_t N, int64_t K) {
  return gemm8_route(Gemm8Entry::Int8Dyn, M, N, K, true, gemm8_force()).kernel != Gemm8Kernel::Invalid ? 1 : 0;
}

extern "C" int ao_int8_dynamic_linear(const uint16_t* x, const int8_t* wq, const float* w_scale, const uint16_t* bias, uint16_t* y,
                                      int64_t M, int64_t N, int64_t K, void* stream) {
  Gemm8Route r;
  if (int rc = check_dyn(__func__, true, M, N, K, &r)) return rc;
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(wq);
  AO_REQUIRE_PTR(w_scale);
  AO_REQUIRE_PTR(y);
  return dyn_linear<true>(r, x, reinterpret_cast<const uint8_t*>(wq), w_scale, bias, y, M, N, K, (hipStream_t)stream);
}

extern "C" int ao_fp8_dynamic_linear(const uint16_t* x, const uint8_t* wq, const float* w_scale, const uint16_t* bias, uint16_t* y,
                                     int64_t M, int64_t N, int64_t K, void* stream) {
  Gemm8Route r;
  if (int rc = check_dyn(__func__, false, M, N, K, &r)) return rc;
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(wq);
  AO_REQUIRE_PTR(w_scale);
  AO_REQUIRE_PTR(y);
  return dyn_linear<false>(r, x, wq, w_scale, bias, y, M, N, K, (hipStream_t)stream);
}
