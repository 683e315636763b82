// The operand staging of the grouped weight-gradient GEMMs (mx_wgrad_kernels.hip, fp8_grouped_train_kernels.hip): 2-D x 2-D grouped
// GEMMs on e4m3 codes stored with the tokens contiguous ([N][M] and [K][M]), 128 x 128 output tiles, k steps on the global 128-token grid.
#pragma once
#include "common.h"

namespace ao {
namespace wgrad_stage {

// Stage layout (that of mx_linear_tile_kernel): g then x, 128 rows each, 128 bytes (one k step of tokens) a row, 16-byte pieces swizzled by
// row so that the 16 lanes of a fragment read hit different banks: piece c of row r sits at slot r * 8 + (c ^ (r % 8)).
constexpr int kOpBytes = 128 * 128;
constexpr int kStage = 2 * kOpBytes;

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, char* lds, uint32_t voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds, 16, voff, 0, 0, 0);
}

__device__ __forceinline__ void wgrad_issue(__amdgpu_buffer_rsrc_t rg, __amdgpu_buffer_rsrc_t rx, char* stage, int n0, int k0, int step, int M,
                                            int N, int K, int wave, int lane) {
  constexpr int kInstr = kOpBytes / 1024;  // 1 KiB per wave instruction
#pragma unroll
  for (int i = wave; i < 2 * kInstr; i += 4) {
    const bool isx = i >= kInstr;
    const int j = isx ? i - kInstr : i;
    const int slot = j * 64 + lane;
    const int r = slot >> 3, c = (slot & 7) ^ (r & 7);
    const int tok = step * 128 + c * 16;
    const int grow = (isx ? k0 : n0) + r;
    const uint32_t voff = (tok < M && grow < (isx ? K : N)) ? (uint32_t)grow * (uint32_t)M + (uint32_t)tok : 0xFFFFFFF0u;
    dma16(isx ? rx : rg, stage + (isx ? kOpBytes : 0) + j * 1024, voff);
  }
}

__device__ __forceinline__ void wgrad_frag(const char* op, int r, int kq, u32x4& v0, u32x4& v1) {
  v0 = *reinterpret_cast<const u32x4*>(op + (r * 8 + (kq ^ (r & 7))) * 16);
  v1 = *reinterpret_cast<const u32x4*>(op + (r * 8 + ((kq + 4) ^ (r & 7))) * 16);
}

// 0xFF in the bytes j < n of a dword
__device__ __forceinline__ uint32_t bytes_below(int n) { return n <= 0 ? 0u : (n >= 4 ? 0xFFFFFFFFu : (1u << (8 * n)) - 1u); }

// 0xFF in the bytes of 16 consecutive tokens from `t0` on that lie in [start, end)
__device__ __forceinline__ u32x4 token_mask(int t0, int start, int end) {
  u32x4 m;
#pragma unroll
  for (int d = 0; d < 4; ++d) m[d] = bytes_below(end - t0 - 4 * d) & ~bytes_below(start - t0 - 4 * d);
  return m;
}

}  // namespace wgrad_stage
}  // namespace ao
