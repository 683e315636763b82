// NVFP4 training casts for gfx950: the operands of the three GEMMs of an NVFP4 linear (e2m1 codes, one e4m3 scale per block of 16, a
// per-tensor amax folded into the encode scale).
//
// Replaces, of torchao's prototype/moe_training/nvfp4_training: triton_rht_amax / cutedsl_rht_amax (hadamard_amax_triton.py),
// triton_rht_quantize_row_col / cutedsl_rht_quantize_row_col (hadamard_quantize_row_col_triton.py) and triton_weight_quantize_2d /
// cutedsl_weight_quantize_2d (quantize_2d_triton.py), which run on sm100 only.  The arithmetic contracts are stated once, in quant_math.h
// ("NVFP4 training").  Scales are written ROW-MAJOR, [rows][cols / 16], which is what the GEMMs of nvfp4_kernels.hip read; the reference's
// 128 x 4 swizzle exists for cuBLAS.
//
// The tile walk of the casts, nvfp4_train_cast_kernel<W2D, SR, GROUPED>, is nvfp4_train_tile.h (shared with the grouped entries of
// nvfp4_grouped_train_kernels.hip); the dense entries here run its GROUPED = false instances.
// nvfp4_train_amax_kernel: a thread holds 16 rows x 2 adjacent columns (one dword a row, a wave 256 contiguous bytes), so both
// 16-point transforms stay in registers; one atomic max a workgroup and output over the non-negative bit patterns.
#include "common.h"
#include "nvfp4_train_tile.h"
#include "quant_math.h"

#include <algorithm>

namespace ao {
namespace {

using namespace nvfp4_train;

__global__ void nvfp4_train_amax_clear_kernel(uint32_t* out2) {
  if (threadIdx.x < 2) out2[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(kThreads) void nvfp4_train_amax_kernel(const uint16_t* __restrict__ x, int64_t M, int64_t N, uint32_t sign_mask,
                                                                    int want_rht, uint32_t* out2) {
  const int64_t half = N >> 1, units = (M >> 4) * half;
  const uint32_t* px = reinterpret_cast<const uint32_t*>(x);
  float mr = 0.f, mc = 0.f;
  for (int64_t unit = (int64_t)blockIdx.x * kThreads + threadIdx.x; unit < units; unit += (int64_t)gridDim.x * kThreads) {
    const int64_t mb = unit / half, c2 = unit - mb * half;
    const uint32_t* pu = px + mb * 16 * half + c2;
    float lo[16], hi[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t w = pu[i * half];
      lo[i] = bf16_lo_to_f32(w);
      hi[i] = bf16_hi_to_f32(w);
    }
    mr = fmaxf(mr, fmaxf(amax16(lo), amax16(hi)));
    if (want_rht) {
      nvfp4_rht16(lo, sign_mask);
      nvfp4_rht16(hi, sign_mask);
      mc = fmaxf(mc, fmaxf(amax16(lo), amax16(hi)));
    }
  }
  // one atomic a workgroup and output, not one a wave: 1024 workgroups then queue 1024 atomics on each of the two addresses, not 4096
  __shared__ float red[2][kThreads / 64];
  mr = wave_max(mr);
  mc = wave_max(mc);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mc;
    red[1][threadIdx.x >> 6] = mr;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    float m = 0.f;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) m = fmaxf(m, red[threadIdx.x][w]);
    if (m > 0.f) atomicMax(out2 + threadIdx.x, f32_to_bits(m));  // (cleared to 0: nothing to add otherwise)
  }
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_nvfp4_train_amax(const uint16_t* x, float* out2, int64_t M, int64_t N, uint32_t sign_mask, int want_rht, void* stream) {
  if (int rc = check_mn(__func__, M, N)) return rc;
  AO_REQUIRE(sign_mask < (1u << 16), "%s: sign_mask must be a 16-bit mask, got 0x%x", __func__, sign_mask);
  AO_REQUIRE_PTR(out2);
  AO_REQUIRE(aligned_to(out2, 4), "%s: out2 must be 4-byte aligned", __func__);
  if (M > 0) {
    AO_REQUIRE_PTR(x);
    AO_REQUIRE(aligned_to(x, 16), "%s: x must be 16-byte aligned", __func__);
  }
  // every check is above: nothing is launched for a call that is refused
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* bits = reinterpret_cast<uint32_t*>(out2);
  ao::launch(nvfp4_train_amax_clear_kernel, dim3(1), dim3(64), 0, s, bits);
  if (M > 0) {
    const int64_t units = (M / 16) * (N / 2);
    const int64_t grid = std::min<int64_t>((units + kThreads - 1) / kThreads, 1024);
    ao::launch(nvfp4_train_amax_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, x, M, N, sign_mask, want_rht, bits);
  }
  AO_LAUNCH_CHECK("nvfp4_train_amax kernels launch");
  return AO_OK;
}

extern "C" int ao_nvfp4_train_quantize_row_col(const uint16_t* x, const float* amax2, uint32_t sign_mask, const int64_t* sr_seed,
                                               const int64_t* col_offset, const int64_t* row_offset, uint8_t* col_q, uint8_t* col_s, uint8_t* row_q,
                                               uint8_t* row_s, int64_t M, int64_t N, void* stream) {
  if (int rc = check_mn(__func__, M, N)) return rc;
  AO_REQUIRE(sign_mask < (1u << 16), "%s: sign_mask must be a 16-bit mask, got 0x%x", __func__, sign_mask);
  AO_REQUIRE((col_q == nullptr) == (col_s == nullptr) && (row_q == nullptr) == (row_s == nullptr),
             "%s: an output's codes and scales are given together or both null", __func__);
  AO_REQUIRE(col_q != nullptr || row_q != nullptr, "%s: both outputs are null", __func__);
  AO_REQUIRE_PTR(amax2);
  if (sr_seed != nullptr) {
    if (col_q != nullptr) AO_REQUIRE_PTR(col_offset);
    if (row_q != nullptr) AO_REQUIRE_PTR(row_offset);
  }
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(col_q, 8) && aligned_to(row_q, 8) && aligned_to(amax2, 4) && aligned_to(sr_seed, 8) &&
                 aligned_to(col_offset, 8) && aligned_to(row_offset, 8),
             "%s: x must be 16-byte, the codes, the seed and the offsets 8-byte and amax2 4-byte aligned", __func__);
  const TrainCastArgs a{x, amax2, amax2 + 1, sign_mask, sr_seed, col_offset, row_offset, col_q, col_s, row_q, row_s, M, N, nullptr, 0};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return sr_seed != nullptr ? launch_cast<false, true, false>(a, 1, st) : launch_cast<false, false, false>(a, 1, st);
}

extern "C" int ao_nvfp4_train_quantize_weight_2d(const uint16_t* w, const float* amax, uint8_t* q, uint8_t* s, uint8_t* qt, uint8_t* st, int64_t N,
                                                 int64_t K, void* stream) {
  if (int rc = check_mn(__func__, N, K)) return rc;
  AO_REQUIRE_PTR(amax);
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(s);
  AO_REQUIRE_PTR(qt);
  AO_REQUIRE_PTR(st);
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(q, 8) && aligned_to(qt, 8) && aligned_to(amax, 4),
             "%s: w must be 16-byte, the codes 8-byte and amax 4-byte aligned", __func__);
  const TrainCastArgs a{w, amax, amax, 0u, nullptr, nullptr, nullptr, qt, st, q, s, N, K, nullptr, 0};
  return launch_cast<true, false, false>(a, 1, static_cast<hipStream_t>(stream));
}
