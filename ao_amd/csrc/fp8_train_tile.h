// The 128 x 128 tile walk of the float8 training casts (fp8_train_kernels.hip, fp8_grouped_train_kernels.hip): 256 threads, a lane holds
// 4 consecutive rows x 8 adjacent columns, the 16 lanes of a DPP row span the tile's 128 columns, the four DPP rows of a wave and the four
// waves stack 16-row slabs, two steps cover the 128 rows.  So a wave owns ONE 16-row slab per step: slab step * 4 + wave of the tile.
#pragma once
#include "common.h"

namespace ao {
namespace fp8_train_tile {

constexpr int kThreads = 256;
constexpr int kTile = 128;
constexpr int kTileLds = 132;  // bytes between two columns of the staged transposed tile

// local row of (step, wave, DPP row, k) and the lane's first column
__device__ __forceinline__ int tile_row(int step, int wave, int g) { return step * 64 + wave * 16 + g * 4; }

__device__ __forceinline__ void unpack8(const u32x4& v, float (&f)[8]) {
  f[0] = bf16_lo_to_f32(v.x); f[1] = bf16_hi_to_f32(v.x); f[2] = bf16_lo_to_f32(v.y); f[3] = bf16_hi_to_f32(v.y);
  f[4] = bf16_lo_to_f32(v.z); f[5] = bf16_hi_to_f32(v.z); f[6] = bf16_lo_to_f32(v.w); f[7] = bf16_hi_to_f32(v.w);
}

}  // namespace fp8_train_tile
}  // namespace ao
