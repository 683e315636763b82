// The weight gradient of the MXFP8 MoE grouped GEMM for gfx950: a 2-D x 2-D grouped GEMM whose contraction runs over each expert's tokens.
//
// Replaces the GEMM of _compute_wgrad (torchao/prototype/moe_training/mxfp8_grouped_mm.py:712-796: torch._scaled_grouped_mm on the 32 x 1
// casts of grad_output and input_act with K-group blocked scales), with the numerics of _emulated_mxfp8_scaled_grouped_mm_2d_2d
// (:1026-1057): both operands dequantised per 32-token block, fp32 accumulation, one rounding to bf16:
//   out[e][n][k] = bf16( sum_{m in [offs[e-1], offs[e])} dq(g)[m][n] dq(x)[m][k] ),  dq = element 2^(scale - 127).
// The operands are what ao_mxfp8_quantize_colwise writes: codes transposed ([N][M_total] and [K][M_total], tokens contiguous) and one scale per
// 32 tokens on the GLOBAL block grid ([M_total/32][rows]), so a row of codes is a row of a dense MX operand whose contraction index is the token
// -- mx_linear_tile_kernel<e4m3> (mx_linear_kernels.hip) with the scales transposed and the k range cut per expert.
//
// mx_wgrad_kernel is the weight-gradient frame (wgrad_frame.h: the grid, the tiles, the stages, the k steps on the global 128-token grid
// and the masks of a step's foreign tokens) with the E8M0 bytes inside the MFMA: a lane's eight scale bytes of a k step (its row of
// every g and x fragment, its 32-token block kq) are loaded while the step before multiplies.  A 32-token block that straddles a group
// boundary lends its scale to both groups and each sums its own tokens.
#include "common.h"
#include "stream_blocks.h"
#include "wgrad_frame.h"

namespace ao {
namespace {

using namespace wgrad_frame;

struct WgradArgs {
  const uint8_t* g;        // e4m3 [N][M]
  const uint8_t* g_scale;  // e8m0 [M/32][N]
  const uint8_t* x;        // e4m3 [K][M]
  const uint8_t* x_scale;  // e8m0 [M/32][K]
  const int32_t* offs;     // [E] cumulative ends; null: one group [0, M)
  uint16_t* out;           // bf16 [E][N][K]
  int M, N, K;
};

struct MxPolicy {
  struct Scales {
    int g[4], x[4];
  };
  const WgradArgs& p;
  const int grow, xrow, kq, mb;  // the lane's row of g's and of x's fragment 0, its 32-token block of a step, the blocks there are
  __device__ __forceinline__ MxPolicy(const WgradArgs& p, const Lane& t, int)
      : p(p), grow(t.n0 + t.wn + t.l16), xrow(t.k0 + t.wk + t.l16), kq(t.kq), mb(p.M >> 5) {}
  // the lane's scale byte of row `row`, 32-token block `blk`: the 16 lanes of a fragment read consecutive bytes
  static __device__ __forceinline__ int scale(const uint8_t* scales, int row, int rows, int blk, int mb) {
    return (row < rows && blk < mb) ? (int)scales[(size_t)blk * rows + row] : 127;
  }
  __device__ __forceinline__ void load(int step, Scales& s) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s.g[i] = scale(p.g_scale, grow + 16 * i, p.N, step * 4 + kq, mb);
      s.x[i] = scale(p.x_scale, xrow + 16 * i, p.K, step * 4 + kq, mb);
    }
  }
  __device__ __forceinline__ f32x4 mac(f32x4 acc, u32x4 g0, u32x4 g1, u32x4 x0, u32x4 x1, const Scales& s, int i, int j) const {
    return mfma8_k128<false, AO_MX_FMT_E4M3>(g0, g1, x0, x1, acc, s.g[i], s.x[j]);
  }
  __device__ __forceinline__ void store(uint16_t* out, const f32x4 (&acc)[4][4], const Lane& t) const {
    wgrad_store<true>(out, t, p.N, p.K, [&](int i, int j, int r, int, int) { return acc[i][j][r]; });
  }
};

__global__ __launch_bounds__(256) void mx_wgrad_kernel(WgradArgs p) {
  wgrad_tile<MxPolicy>(p);
}

// dense: one group [0, M_total) and no offs tensor (E == 1)
int wgrad(const char* fn, const uint8_t* g_t, const uint8_t* g_scale, const uint8_t* x_t, const uint8_t* x_scale, const int32_t* offs, uint16_t* out,
          int64_t M_total, int64_t N, int64_t K, int64_t E, bool dense, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  bool launch;
  if (int rc = check_entry(Entry{fn, "M_total", 32, 16, dense}, g_t, x_t, offs, out, M_total, N, K, E, st, &launch)) return rc;
  if (!launch) return AO_OK;
  AO_REQUIRE_PTR_FN(fn, g_scale);
  AO_REQUIRE_PTR_FN(fn, x_scale);
  const WgradArgs args{g_t, g_scale, x_t, x_scale, dense ? nullptr : offs, out, (int)M_total, (int)N, (int)K};
  return launch_frame(mx_wgrad_kernel, "mx_wgrad_kernel", args, N, K, E, st);
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_mxfp8_grouped_mm_wgrad(const uint8_t* g_t, const uint8_t* g_scale, const uint8_t* x_t, const uint8_t* x_scale,
                                         const int32_t* offs, uint16_t* out, int64_t M_total, int64_t N, int64_t K, int64_t E, void* stream) {
  return wgrad(__func__, g_t, g_scale, x_t, x_scale, offs, out, M_total, N, K, E, false, stream);
}

extern "C" int ao_mxfp8_mm_wgrad(const uint8_t* g_t, const uint8_t* g_scale, const uint8_t* x_t, const uint8_t* x_scale, uint16_t* out, int64_t M,
                                 int64_t N, int64_t K, void* stream) {
  return wgrad(__func__, g_t, g_scale, x_t, x_scale, nullptr, out, M, N, K, 1, true, stream);
}
