// The 128 x 128 tile walk of the float8 training casts (fp8_train_kernels.hip, fp8_grouped_train_kernels.hip, fp8_block_train_kernels.hip):
// 256 threads, a lane holds 4 consecutive rows x 8 adjacent columns (four 16-byte loads), the 16 lanes of a DPP row span the tile's 128
// columns, the four DPP rows of a wave and the four waves stack 16-row slabs, two steps cover the 128 rows.  So a wave owns ONE 16-row
// slab per step: slab step * 4 + wave of the tile.  With lane = 16 g + ci:
//   * a row's 8 codes leave as one 8-byte store, 128 contiguous bytes per DPP row;
//   * a column's 4 codes of a lane are one cvt4_e4m3 dword, staged in LDS (stage_cols_t; column stride 132 B: 2-way bank conflicts on
//     the write, like mxfp8_quant_colwise_kernel) and read back so that every column leaves as 128-byte runs of the transposed output
//     (flush_cols_t);
//   * the row amax is a DPP reduction over 16 lanes (row16_max), the column amax two shuffles (reduce_cols) and one LDS step across the
//     waves or slabs, which is the kernel's.
// The helpers move data; the arithmetic is quant_math.h's (fp8_train_q).
#pragma once
#include "common.h"
#include "quant_math.h"

namespace ao {
namespace fp8_train_tile {

constexpr int kThreads = 256;
constexpr int kTile = 128;
constexpr int kTileLds = 132;  // bytes between two columns of the staged transposed tile
constexpr int kTileLdsBytes = kTile * kTileLds;  // the staged tile

// local row of (step, wave, DPP row, k) and the lane's first column
__device__ __forceinline__ int tile_row(int step, int wave, int g) { return step * 64 + wave * 16 + g * 4; }

__device__ __forceinline__ void unpack8(const u32x4& v, float (&f)[8]) {
  f[0] = bf16_lo_to_f32(v.x); f[1] = bf16_hi_to_f32(v.x); f[2] = bf16_lo_to_f32(v.y); f[3] = bf16_hi_to_f32(v.y);
  f[4] = bf16_lo_to_f32(v.z); f[5] = bf16_hi_to_f32(v.z); f[6] = bf16_lo_to_f32(v.w); f[7] = bf16_hi_to_f32(v.w);
}

// The lane's part of the tile at row r0 of x [R][C], its columns c .. c + 7: rows past R read as zeros, and (COL_GUARD) so do columns
// past C -- a lane's 8 columns are inside together (C % 8 == 0).
template <bool COL_GUARD>
__device__ __forceinline__ void load_tile(const uint16_t* x, int64_t r0, int64_t c, int64_t R, int64_t C, int wave, int g,
                                          u32x4 (&v)[2][4]) {
#pragma unroll
  for (int step = 0; step < 2; ++step)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t r = r0 + tile_row(step, wave, g) + k;
      v[step][k] = (r < R && (!COL_GUARD || c < C)) ? *reinterpret_cast<const u32x4*>(x + r * C + c) : u32x4{0u, 0u, 0u, 0u};
    }
}

// A lane's 8 column maxima merged over the four DPP rows of its wave; DPP row 0 writes the wave's 128 into cred_row.
__device__ __forceinline__ void reduce_cols(float (&cm)[8], float* cred_row, int ci, int g) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    cm[j] = fmaxf(cm[j], __shfl_xor(cm[j], 16));
    cm[j] = fmaxf(cm[j], __shfl_xor(cm[j], 32));
  }
  if (g == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) cred_row[8 * ci + j] = cm[j];
  }
}

// The codes of a step's 4 rows (local rows lr .. lr + 3) x the lane's 8 columns into the transposed tile [kTile][kTileLds]: one dword
// a column (lr % 4 == 0, 132 % 4 == 0), column j on the scale sc[j]; !live: zeros.
__device__ __forceinline__ void stage_cols_t(uint8_t* tile, const u32x4 (&v)[4], const float (&sc)[8], int ci, int lr, bool live = true) {
  float f[4][8];
#pragma unroll
  for (int k = 0; k < 4; ++k) unpack8(v[k], f[k]);
#pragma unroll
  for (int j = 0; j < 8; ++j)
    *reinterpret_cast<uint32_t*>(tile + (8 * ci + j) * kTileLds + lr) =
        live ? cvt4_e4m3(fp8_train_q(f[0][j], sc[j]), fp8_train_q(f[1][j], sc[j]), fp8_train_q(f[2][j], sc[j]), fp8_train_q(f[3][j], sc[j]))
             : 0u;
}

// The staged tile leaves as 128 columns x 8 pieces of 16 bytes (16 rows each): the piece of column gc = c0 + col from row gr = r0 + 16 part
// on goes to dst(gc, gr).  CHECKED: only pieces that start inside [C][R] (R % 16 == 0: such a piece lies inside).
template <bool CHECKED, class Dst>
__device__ __forceinline__ void flush_cols_t(const uint8_t* tile, int64_t c0, int64_t r0, int64_t C, int64_t R, Dst dst) {
  for (int p = threadIdx.x; p < kTile * 8; p += kThreads) {
    const int col = p >> 3, part = p & 7;
    const int64_t gc = c0 + col, gr = r0 + part * 16;
    if (!CHECKED || (gc < C && gr < R)) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(tile + col * kTileLds + part * 16);
      *reinterpret_cast<u32x4*>(dst(gc, gr)) = u32x4{src[0], src[1], src[2], src[3]};
    }
  }
}

}  // namespace fp8_train_tile
}  // namespace ao
