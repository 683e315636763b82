// float8 TRAINING casts for gfx950: the dynamic casts of torchao.float8 (hp_tensor_to_float8_dynamic), one scale per row, per column
// or per tensor, codes row-major and / or transposed.  The arithmetic is stated once, in quant_math.h (fp8_train_scale, fp8_train_q).
//
// Reference (torchao 0.19.0 snapshot):
//   scale : float8/float8_utils.py:31-53 (amax_to_scale: float64 division), :244-246 (round down to a power of two)
//   amax  : float8/float8_utils.py:56-82 (tensor_to_amax: max |x| over the tensor or along one axis)
//   cast  : float8/float8_training_tensor.py:153-154 (f32(x) * scale), float8/float8_utils.py:118-139 (saturated cast)
//   1/s   : float8/float8_ops.py:44-45 (the GEMM takes scale.reciprocal())
//
// Two passes over x serve any set of directions: ao_fp8_train_amax reads x once for the row and / or column maxima, ao_fp8_train_cast
// reads it once more and writes the row-major codes and / or the transposed ones.  Both walk 128 x 128 tiles with the register layout
// and the helpers of fp8_train_tile.h.
// Tile edges: C % 8 == 0 keeps a lane's 8 columns inside together; rows are checked one by one; the transposed output needs
// R % 16 == 0 (its 16-byte pieces, and the K of the GEMM that reads it).
#include "common.h"
#include "quant_math.h"
#include "fp8_train_tile.h"

namespace ao {
namespace {

using namespace fp8_train_tile;  // the constants and the helpers of the tile walk

// ---- amax: one read of x; partial maxima of a tile merge into the zeroed outputs by an unsigned atomic max (non-negative fp32 order
// like their bit patterns), so the result does not depend on the order the tiles arrive in ------------------------------------------------
template <bool ROWS, bool COLS>
__global__ __launch_bounds__(kThreads) void fp8_train_amax_kernel(const uint16_t* __restrict__ x, float* __restrict__ row_amax,
                                                                  float* __restrict__ col_amax, int64_t R, int64_t C) {
  __shared__ float cred[4][kTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.y * kTile, c = (int64_t)blockIdx.x * kTile + 8 * ci;
  u32x4 v[2][4];
  load_tile<true>(x, r0, c, R, C, wave, g, v);
  float cm[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int step = 0; step < 2; ++step)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float f[8];
      unpack8(v[step][k], f);
      float rm = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a = fabsf(f[j]);
        rm = fmaxf(rm, a);
        cm[j] = fmaxf(cm[j], a);
      }
      if (ROWS) {
        rm = row16_max(rm);
        const int64_t r = r0 + tile_row(step, wave, g) + k;
        if (ci == 0 && r < R) atomicMax(reinterpret_cast<unsigned int*>(row_amax + r), f32_to_bits(rm));
      }
    }
  if (COLS) {
    reduce_cols(cm, cred[wave], ci, g);
    __syncthreads();
    const int64_t gc = (int64_t)blockIdx.x * kTile + threadIdx.x;
    if (threadIdx.x < kTile && gc < C) {
      const int t = threadIdx.x;
      const float m = fmaxf(fmaxf(cred[0][t], cred[1][t]), fmaxf(cred[2][t], cred[3][t]));
      atomicMax(reinterpret_cast<unsigned int*>(col_amax + gc), f32_to_bits(m));
    }
  }
}

// ---- cast: one read of x, the codes of either or both directions ---------------------------------------------------------------------------
// The tile's 128 row scales and 128 column scales are made once, one float64 division per thread, and shared through LDS; the tiles of
// the first column (row) of the grid write them out with their reciprocals.  An amax stride of 0: one amax for the whole tensor.
template <bool ROWS, bool COLS>
__global__ __launch_bounds__(kThreads) void fp8_train_cast_kernel(const uint16_t* __restrict__ x, const float* __restrict__ row_amax,
                                                                  int64_t row_stride, const float* __restrict__ col_amax,
                                                                  int64_t col_stride, int pow2, uint8_t* __restrict__ q_row,
                                                                  float* __restrict__ s_row, float* __restrict__ inv_s_row,
                                                                  uint8_t* __restrict__ q_col_t, float* __restrict__ s_col,
                                                                  float* __restrict__ inv_s_col, int64_t R, int64_t C) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[COLS ? kTileLdsBytes : 16];
  __shared__ float rs[kTile], cs[kTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.y * kTile, c0 = (int64_t)blockIdx.x * kTile, c = c0 + 8 * ci;
  u32x4 v[2][4];
  load_tile<true>(x, r0, c, R, C, wave, g, v);
  if (threadIdx.x < kTile) {
    if (COLS) {
      const int64_t gc = c0 + threadIdx.x;
      float s = 0.f;
      if (gc < C) {
        s = fp8_train_scale(col_amax[gc * col_stride], pow2 != 0);
        if (blockIdx.y == 0) {
          s_col[gc] = s;
          inv_s_col[gc] = 1.0f / s;
        }
      }
      cs[threadIdx.x] = s;
    }
  } else if (ROWS) {
    const int t = threadIdx.x - kTile;
    const int64_t gr = r0 + t;
    float s = 0.f;
    if (gr < R) {
      s = fp8_train_scale(row_amax[gr * row_stride], pow2 != 0);
      if (blockIdx.x == 0) {
        s_row[gr] = s;
        inv_s_row[gr] = 1.0f / s;
      }
    }
    rs[t] = s;
  }
  __syncthreads();
  float sc[8];
  if (COLS) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sc[j] = cs[8 * ci + j];
  }
#pragma unroll
  for (int step = 0; step < 2; ++step) {
    const int lr = tile_row(step, wave, g);
    if (ROWS) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t r = r0 + lr + k;
        if (r < R && c < C) *reinterpret_cast<u32x2*>(q_row + r * C + c) = fp8_train_quant8(v[step][k], rs[lr + k]);
      }
    }
    if (COLS) stage_cols_t(tile, v[step], sc, ci, lr);
  }
  if (COLS) {
    __syncthreads();
    flush_cols_t<true>(tile, c0, r0, C, R, [&](int64_t gc, int64_t gr) { return q_col_t + gc * R + gr; });
  }
}

// ---- the row-only cast as ONE launch: a workgroup per row, amax and cast from the same registers (C <= 16384; longer rows take a
// second sweep, through L2).  NV = 16-byte vectors per thread, 0 = the two-sweep form.  fp8_quant_rowwise_kernel / quant_rowwise_reg_kernel
// with the training arithmetic: the bytes of ao_fp8_train_amax + ao_fp8_train_cast.
template <int NV>
__global__ __launch_bounds__(kThreads) void fp8_train_quant_rowwise_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q,
                                                                           float* __restrict__ s_out, float* __restrict__ inv_s_out,
                                                                           int pow2, int64_t C) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const u32x4* xr = reinterpret_cast<const u32x4*>(x + row * C);
  u32x2* qr = reinterpret_cast<u32x2*>(q + row * C);
  const int64_t nvec = C >> 3;
  constexpr int NR = NV > 0 ? NV : 1;
  u32x4 v[NR];
  float m = 0.f;
  bool has_nan = false;  // (non-finite inputs are outside the contract; amax8 asks for the flag)
  if (NV > 0) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int64_t idx = threadIdx.x + i * kThreads;
      v[i] = (idx < nvec) ? xr[idx] : u32x4{0u, 0u, 0u, 0u};
      m = fmaxf(m, amax8(v[i], has_nan));
    }
  } else {
    for (int64_t i = threadIdx.x; i < nvec; i += kThreads) m = fmaxf(m, amax8(xr[i], has_nan));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float s = fp8_train_scale(m, pow2 != 0);
  if (threadIdx.x == 0) {
    s_out[row] = s;
    inv_s_out[row] = 1.0f / s;
  }
  if (NV > 0) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int64_t idx = threadIdx.x + i * kThreads;
      if (idx < nvec) qr[idx] = fp8_train_quant8(v[i], s);
    }
  } else {
    for (int64_t i = threadIdx.x; i < nvec; i += kThreads) qr[i] = fp8_train_quant8(xr[i], s);
  }
}

int check_shape(const char* fn, int64_t R, int64_t C, bool transposed) {
  AO_REQUIRE(R >= 0 && C >= 0, "%s: bad shape R=%lld C=%lld", fn, (long long)R, (long long)C);
  AO_REQUIRE(C % 16 == 0, "%s: C=%lld must be a multiple of 16", fn, (long long)C);
  AO_REQUIRE(!transposed || R % 16 == 0, "%s: R=%lld must be a multiple of 16 for the transposed output (its rows are the GEMM's K)", fn,
             (long long)R);
  AO_REQUIRE((R + kTile - 1) / kTile <= 65535 && (C + kTile - 1) / kTile < (1ll << 31), "%s: R=%lld C=%lld too large for one launch", fn,
             (long long)R, (long long)C);
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_fp8_train_amax(const uint16_t* x, float* row_amax, float* col_amax, int64_t R, int64_t C, void* stream) {
  if (int rc = check_shape(__func__, R, C, false)) return rc;
  if (R == 0 || C == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE(row_amax != nullptr || col_amax != nullptr, "%s: neither row_amax nor col_amax given", __func__);
  hipStream_t s = (hipStream_t)stream;
  if (row_amax != nullptr) {
    const hipError_t e = hipMemsetAsync(row_amax, 0, (size_t)R * sizeof(float), s);
    if (e != hipSuccess) return hip_failed(e, "ao_fp8_train_amax: zeroing row_amax");
  }
  if (col_amax != nullptr) {
    const hipError_t e = hipMemsetAsync(col_amax, 0, (size_t)C * sizeof(float), s);
    if (e != hipSuccess) return hip_failed(e, "ao_fp8_train_amax: zeroing col_amax");
  }
  const dim3 grid((unsigned)((C + kTile - 1) / kTile), (unsigned)((R + kTile - 1) / kTile)), block(kThreads);
  if (row_amax != nullptr && col_amax != nullptr) ao::launch(fp8_train_amax_kernel<true, true>, grid, block, 0, s, x, row_amax, col_amax, R, C);
  else if (row_amax != nullptr) ao::launch(fp8_train_amax_kernel<true, false>, grid, block, 0, s, x, row_amax, col_amax, R, C);
  else ao::launch(fp8_train_amax_kernel<false, true>, grid, block, 0, s, x, row_amax, col_amax, R, C);
  AO_LAUNCH_CHECK("fp8_train_amax_kernel launch");
  return AO_OK;
}

extern "C" int ao_fp8_train_cast(const uint16_t* x, const float* row_amax, int64_t row_amax_stride, const float* col_amax,
                                 int64_t col_amax_stride, int pow2, uint8_t* q_row, float* s_row, float* inv_s_row, uint8_t* q_col_t,
                                 float* s_col, float* inv_s_col, int64_t R, int64_t C, void* stream) {
  const bool rows = q_row != nullptr, cols = q_col_t != nullptr;
  if (int rc = check_shape(__func__, R, C, cols)) return rc;
  AO_REQUIRE((row_amax_stride == 0 || row_amax_stride == 1) && (col_amax_stride == 0 || col_amax_stride == 1),
             "%s: an amax stride is 1 (one per row / column) or 0 (one for the tensor), got %lld and %lld", __func__,
             (long long)row_amax_stride, (long long)col_amax_stride);
  if (R == 0 || C == 0) return AO_OK;
  AO_REQUIRE(rows || cols, "%s: neither q_row nor q_col_t given", __func__);
  AO_REQUIRE_PTR(x);
  if (rows) {
    AO_REQUIRE_PTR(row_amax);
    AO_REQUIRE_PTR(s_row);
    AO_REQUIRE_PTR(inv_s_row);
  }
  if (cols) {
    AO_REQUIRE_PTR(col_amax);
    AO_REQUIRE_PTR(s_col);
    AO_REQUIRE_PTR(inv_s_col);
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((C + kTile - 1) / kTile), (unsigned)((R + kTile - 1) / kTile)), block(kThreads);
#define AO_FP8_TRAIN_CAST(RW, CL)                                                                                                   \
  ao::launch(fp8_train_cast_kernel<RW, CL>, grid, block, 0, s, x, row_amax, row_amax_stride, col_amax, col_amax_stride, pow2, q_row, \
             s_row, inv_s_row, q_col_t, s_col, inv_s_col, R, C)
  if (rows && cols) AO_FP8_TRAIN_CAST(true, true);
  else if (rows) AO_FP8_TRAIN_CAST(true, false);
  else AO_FP8_TRAIN_CAST(false, true);
#undef AO_FP8_TRAIN_CAST
  AO_LAUNCH_CHECK("fp8_train_cast_kernel launch");
  return AO_OK;
}

extern "C" int ao_fp8_train_quantize_rowwise(const uint16_t* x, uint8_t* q, float* s, float* inv_s, int pow2, int64_t R, int64_t C,
                                             void* stream) {
  if (int rc = check_shape(__func__, R, C, false)) return rc;
  AO_REQUIRE(R < (1ll << 31), "%s: R=%lld too large", __func__, (long long)R);
  if (R == 0 || C == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(s);
  AO_REQUIRE_PTR(inv_s);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)R), block(kThreads);
  static_assert(kThreads == kRowThreads, "with_row_depth sizes NV for kRowThreads threads");
  auto go = [&](auto nv) { ao::launch(fp8_train_quant_rowwise_kernel<decltype(nv)::value>, grid, block, 0, st, x, q, s, inv_s, pow2, C); };
  if (!with_row_depth(C, go)) go(std::integral_constant<int, 0>{});  // longer rows: the walking form
  AO_LAUNCH_CHECK("fp8_train_quant_rowwise_kernel launch");
  return AO_OK;
}
