// SmoothQuant for gfx950: the two calibration reductions.  (The int8 activation casts with the smoothing pre-scale folded in are the PRE = true
// instantiations of the casts in quant_kernels.hip, and their entry points live there.)
//
// Reference (torchao 0.19.0 snapshot): prototype/smoothquant/core.py:41-75 (x_abs_max, w_abs_max, the amax of example_input / smoothing_factor),
// :162-206 (the running observer's two passes).  Both kernels are bandwidth-bound streams of 16-byte loads.
//
//   A  ao_sq_col_absmax_update      state[k] = max(state[k], max_m |x[m,k]|)                    fp32 [K], in place
//   B  ao_sq_smoothed_amax_update   amax     = max(amax, max_mk |bf16(f32(x[m,k]) / f32(s[k]))|)  fp32 [1], in place
//
// A and B fold into their state with atomicMax on the BIT PATTERN: a non-negative float's bits order as unsigned integers, every operand is
// non-negative (|.| clears the sign, so -0.0 counts as 0) and max is exact, so the result does not depend on the order in which workgroups
// arrive: two launches give the same bytes.  The state must hold non-negative floats (zeros before the first update).  NaN and Inf inputs are
// outside the contract, as in the casts.
//
// A: a workgroup owns 512 columns (64 lanes x one 16-byte slice) and a range of rows; its four waves take different rows, four rows in flight
// each, and a lane keeps the eight running maxima of its slice as packed bf16 bit patterns (v_pk_max_u16 on |x|: the same ordering argument).
// The waves meet in LDS, then thread t owns columns t and t + 256 of the tile, so that every atomic wave-instruction covers 256 contiguous
// bytes of `state` (the shape the memory-side atomics run fastest at); zeros are not sent.  The row range is split so that about 2048
// workgroups exist however small K / 512 is.
// B: a thread owns one 16-byte column slice, keeps its eight divisors in registers and walks rows; IEEE division (hipcc's default for fp32
// `/`, no fast reciprocal), one rounding to bf16, a block reduction and ONE atomic per workgroup.
#include <algorithm>

#include "common.h"
#include "quant_math.h"

namespace ao {
namespace {

constexpr int kThreads = kRowThreads;  // (block_max: common.h)
constexpr int kColTile = 512;     // kernel A: columns per workgroup
constexpr int kRowsInFlight = 4;  // kernel A: rows a wave has in flight
constexpr int64_t kTargetBlocks = 2048;  // 8 per CU

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

// running packed |bf16| maxima of a 16-byte slice
__device__ __forceinline__ void absmax8_update(u32x4& m, const u32x4& v) {
  m.x = pk_max_u16(m.x, v.x & 0x7fff7fffu);
  m.y = pk_max_u16(m.y, v.y & 0x7fff7fffu);
  m.z = pk_max_u16(m.z, v.z & 0x7fff7fffu);
  m.w = pk_max_u16(m.w, v.w & 0x7fff7fffu);
}

// ---- A: running per-column absmax ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sq_col_absmax_kernel(const uint16_t* __restrict__ x, uint32_t* __restrict__ state, int64_t M, int64_t K,
                                                                 int64_t rows_per_block) {
  __shared__ __attribute__((aligned(16))) uint16_t red[kThreads / 64][kColTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * kColTile;
  const int64_t c = c0 + lane * 8;  // K % 8 == 0: a slice that starts inside a row ends inside it
  const int64_t r_begin = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r_end = r_begin + rows_per_block < M ? r_begin + rows_per_block : M;
  u32x4 m = {0u, 0u, 0u, 0u};
  if (c < K) {
    constexpr int kStep = (kThreads / 64) * kRowsInFlight;
    for (int64_t r = r_begin + wave; r < r_end; r += kStep) {
      u32x4 v[kRowsInFlight];
#pragma unroll
      for (int j = 0; j < kRowsInFlight; ++j) {
        const int64_t rj = r + j * (kThreads / 64);
        v[j] = rj < r_end ? *reinterpret_cast<const u32x4*>(x + rj * K + c) : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int j = 0; j < kRowsInFlight; ++j) absmax8_update(m, v[j]);
    }
  }
  *reinterpret_cast<u32x4*>(&red[wave][lane * 8]) = m;
  __syncthreads();
#pragma unroll
  for (int h = 0; h < kColTile / kThreads; ++h) {
    const int col = threadIdx.x + h * kThreads;
    uint16_t b = red[0][col];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) b = red[w][col] > b ? red[w][col] : b;
    if (c0 + col < K && b != 0) atomicMax(state + c0 + col, (uint32_t)b << 16);  // fp32 bits of a bf16 value
  }
}

// ---- B: running amax of the smoothed activation -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sq_smoothed_amax_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ s,
                                                                    uint32_t* __restrict__ amax, int64_t M, int64_t K, int64_t rows_per_block) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  const int64_t c = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 8;
  const int64_t r_begin = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r_end = r_begin + rows_per_block < M ? r_begin + rows_per_block : M;
  float m = 0.f;
  if (c < K) {
    float d[8], f[8];
    unpack_bf16x8(*reinterpret_cast<const u32x4*>(s + c), d);
#pragma unroll 2
    for (int64_t r = r_begin; r < r_end; ++r) {
      unpack_bf16x8(*reinterpret_cast<const u32x4*>(x + r * K + c), f);
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const float a = round_bf16(f[j] / d[j]), b = round_bf16(f[j + 1] / d[j + 1]);
        m = fmaxf(m, fmaxf(fabsf(a), fabsf(b)));
      }
    }
  }
  m = block_max(m, red);
  if (threadIdx.x == 0 && m != 0.f) atomicMax(amax, f32_to_bits(m));
}

// rows per workgroup so that about kTargetBlocks workgroups exist over `col_blocks` column tiles; at least `min_rows` rows each
int64_t rows_per_block(int64_t M, int64_t col_blocks, int64_t min_rows) {
  const int64_t splits = std::max<int64_t>(1, std::min<int64_t>(kTargetBlocks / col_blocks, (M + min_rows - 1) / min_rows));
  return (M + splits - 1) / splits;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_sq_col_absmax_update(const uint16_t* x, float* state, int64_t M, int64_t K, void* stream) {
  if (int rc = check_rows(__func__, M, K, 8)) return rc;
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(state);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(state, 4), "%s: x must be 16-byte aligned and state 4-byte aligned", __func__);
  const int64_t gx = (K + kColTile - 1) / kColTile;
  const int64_t rows = rows_per_block(M, gx, (kThreads / 64) * kRowsInFlight);
  const int64_t gy = (M + rows - 1) / rows;
  ao::launch(sq_col_absmax_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), 0, (hipStream_t)stream, x,
             reinterpret_cast<uint32_t*>(state), M, K, rows);
  AO_LAUNCH_CHECK("sq_col_absmax_kernel launch");
  return AO_OK;
}

extern "C" int ao_sq_smoothed_amax_update(const uint16_t* x, const uint16_t* s, float* amax, int64_t M, int64_t K, void* stream) {
  if (int rc = check_rows(__func__, M, K, 8)) return rc;
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(s);
  AO_REQUIRE_PTR(amax);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(s, 16) && aligned_to(amax, 4), "%s: x and s must be 16-byte aligned and amax 4-byte aligned", __func__);
  const int64_t gx = ((K >> 3) + kThreads - 1) / kThreads;
  const int64_t rows = rows_per_block(M, gx, 1);
  const int64_t gy = (M + rows - 1) / rows;
  ao::launch(sq_smoothed_amax_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), 0, (hipStream_t)stream, x, s,
             reinterpret_cast<uint32_t*>(amax), M, K, rows);
  AO_LAUNCH_CHECK("sq_smoothed_amax_kernel launch");
  return AO_OK;
}
