// Blockwise float8 TRAINING for gfx950 (the DeepSeek-V3 recipe): the block-local casts and the weight-gradient GEMM of
// torchao/prototype/blockwise_fp8_training (linear.py: fp8_blockwise_mm).  The forward and the input gradient are ao_fp8_block_linear
// (fp8_block_kernels.hip) on these casts: its chain acc += (p * a_s) * b_s is triton_fp8_gemm_1x128_128x128's (kernels.py:197-260).
//
// The casts (contract: the torch_blockwise_scale_* functions, kernels.py:1031-1156, which tests/golden/blockwise_fp8_training.npz records):
//   scale = f32(448 / max(f64(amax_block), 1e-12));  q = e4m3(clamp(f32(x) * scale, -448, 448));  the GEMMs take inv = 1 / scale.
// This is the float8 training cast's arithmetic, stated once in quant_math.h (fp8_train_scale(amax, false), fp8_train_q) -- NOT the
// inference block cast of fp8_block_kernels.hip (scale = bf16(amax / 448), q = x / scale): there a block of zeros gives scale 0 and NaN
// codes, here it gives scale f32(448 / 1e-12), codes 0 and no NaN.
//   One difference between the directions, taken from the reference as it is: torch_blockwise_scale_act_quant_rhs (128 x 1 blocks)
//   clamps the amax at 1e-12 BEFORE it widens it to float64, i.e. in bf16, where 1e-12 is 0x2B8D = 1.00186e-12 (kernels.py:1096; the
//   Triton casts clamp there too); the 1 x 128 and 128 x 128 functions widen first (:1043-1044, :1140-1141).  Only the reciprocal of a
//   block whose amax is below 1.00186e-12 can tell the two apart (its codes are 0 either way: 448e-12 * 1e-12-sized inputs round to 0).
//
// fp8_block_train_cast_kernel walks 128 x 128 tiles with the register layout of fp8_train_tile.h.  A tile holds whole blocks in every
// direction, so no amax pre-pass: the 128 row maxima (DPP rows), the 128 column maxima (two shuffles and one LDS step across the waves)
// or the tile's maximum meet in LDS, one thread a scale makes the float64 division and writes the reciprocal, and the codes leave as in
// fp8_train_cast_kernel: 8 bytes a lane for the row-major output, 128-byte runs through an LDS transposition for the transposed one.
// No allocation, no synchronisation, no atomics.
//
// fp8_block_wgrad_kernel (ao_fp8_block_mm_wgrad; kernels.py:320-379, triton_fp8_gemm_1x128_128x1): out[n][k] = bf16(sum over token
// blocks mb, ascending, of (p * g_inv[mb][n]) * x_inv[mb][k]), p = the block's 128 tokens as ONE scaled MFMA onto a zero accumulator.
// mx_wgrad_kernel's frame: 128 x 128 output tiles, four waves of 64 x 64, operands staged by wgrad_stage.h in two stages; the scale
// vectors of step mb + 1 (128 contiguous floats each per tile) are loaded into registers while step mb multiplies.  A lane's rows
// 4 kq + r take g_inv as fp8_block_acc's a_s; its column is fixed per j, so x_inv is fp8_block_acc's b_s, one value per lane.  No split
// along the tokens: a launch is reproducible.
//
// The routed experts (torchao/prototype/moe_training/blockwise_fp8/grouped_mm.py:98-265): the weight cast over a stack of
// experts is the same cast kernel with the expert in blockIdx.z (ao_fp8_block_train_cast_weight_3d), and fp8_block_grouped_wgrad_kernel
// (ao_fp8_block_grouped_mm_wgrad) is the weight gradient per token group on the same column casts of all tokens.
#include "common.h"
#include "quant_math.h"
#include "stream_blocks.h"
#include "fp8_train_tile.h"
#include "wgrad_stage.h"

namespace ao {
namespace {

using namespace fp8_train_tile;  // kThreads, kTile, kTileLds, tile_row, unpack8

// 1e-12 rounded to bf16: where torch.clamp(amax_bf16, min=1e-12) puts a smaller amax (the 128 x 1 direction)
constexpr uint32_t kEpsBf16Bits = 0x2B8D0000u;

// ---- the casts ----------------------------------------------------------------------------------------------------------------------------
// WEIGHT false: ROWS = 1 x 128 blocks (q_row [R][C], inv_row [R][C/128]), COLS = 128 x 1 blocks stored transposed (q_col_t [C][R],
//               inv_col [R/128][C]).
// WEIGHT true : one 128 x 128 block a tile; ROWS = the plain layout (q_row [R][C], inv_row [R/128][C/128]), COLS = the transposed one
//               (q_col_t [C][R], inv_col [C/128][R/128]).
// C % 128 == 0 always; rows past R (ROWS only, not WEIGHT) are read as zeros and never stored.
// BATCHED (WEIGHT only): a 3-D weight [E][R][C], expert blockIdx.z.  Every layout of an expert is the 2-D one at the expert's offset (R and C
//               are multiples of 128, so a block never holds two experts): the walk is the 2-D walk on pointers moved to the expert.
template <bool ROWS, bool COLS, bool WEIGHT, bool BATCHED = false>
__global__ __launch_bounds__(kThreads) void fp8_block_train_cast_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q_row,
                                                                        float* __restrict__ inv_row, uint8_t* __restrict__ q_col_t,
                                                                        float* __restrict__ inv_col, int64_t R, int64_t C) {
  constexpr bool kRowMax = ROWS || WEIGHT, kColMax = COLS && !WEIGHT;
  __shared__ __attribute__((aligned(16))) uint8_t tile[COLS ? kTile * kTileLds : 16];
  __shared__ float rs[kTile], cs[kTile];  // the maxima, then the scales
  __shared__ float cred[kColMax ? 4 : 1][kTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.y * kTile, c0 = (int64_t)blockIdx.x * kTile, c = c0 + 8 * ci;
  if (BATCHED) {
    static_assert(WEIGHT || !BATCHED, "the batched walk is the weight cast's");
    const int64_t e = blockIdx.z, blocks = (R / kTile) * (C / kTile);
    x += e * R * C;
    if (ROWS) {
      q_row += e * R * C;
      inv_row += e * blocks;
    }
    if (COLS) {
      q_col_t += e * R * C;
      inv_col += e * blocks;
    }
  }
  u32x4 v[2][4];
#pragma unroll
  for (int step = 0; step < 2; ++step)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t r = r0 + tile_row(step, wave, g) + k;
      v[step][k] = r < R ? *reinterpret_cast<const u32x4*>(x + r * C + c) : u32x4{0u, 0u, 0u, 0u};
    }
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
      if (kRowMax) {
        rm = row16_max(rm);
        if (ci == 0) rs[tile_row(step, wave, g) + k] = rm;
      }
    }
  if (kColMax) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      cm[j] = fmaxf(cm[j], __shfl_xor(cm[j], 16));
      cm[j] = fmaxf(cm[j], __shfl_xor(cm[j], 32));
    }
    if (g == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) cred[wave][8 * ci + j] = cm[j];
    }
  }
  __syncthreads();
  if (WEIGHT) {
    // the tile's maximum from the 128 row maxima, in every lane of every wave; thread 0 divides
    const float m = wave_max(fmaxf(rs[lane], rs[lane + 64]));
    if (threadIdx.x == 0) {
      const float s = fp8_train_scale(m, false);
      cs[0] = s;
      if (ROWS) inv_row[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = 1.0f / s;
      if (COLS) inv_col[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = 1.0f / s;
    }
  } else if (threadIdx.x < kTile) {
    if (COLS) {
      const int t = threadIdx.x;
      const float m = fmaxf(fmaxf(cred[0][t], cred[1][t]), fmaxf(cred[2][t], cred[3][t]));
      const float s = fp8_train_scale(fmaxf(m, bits_to_f32(kEpsBf16Bits)), false);  // (the clamp in bf16 first: see the header)
      inv_col[(int64_t)blockIdx.y * C + c0 + t] = 1.0f / s;
      cs[t] = s;
    }
  } else if (ROWS) {
    const int t = threadIdx.x - kTile;
    const float s = fp8_train_scale(rs[t], false);
    if (r0 + t < R) inv_row[(r0 + t) * (C / kTile) + blockIdx.x] = 1.0f / s;
    rs[t] = s;
  }
  __syncthreads();
  const float ws = WEIGHT ? cs[0] : 0.f;
  float sc[8];
  if (COLS) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sc[j] = WEIGHT ? ws : cs[8 * ci + j];
  }
#pragma unroll
  for (int step = 0; step < 2; ++step) {
    const int lr = tile_row(step, wave, g);
    if (ROWS) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t r = r0 + lr + k;
        if (r < R) *reinterpret_cast<u32x2*>(q_row + r * C + c) = fp8_train_quant8(v[step][k], WEIGHT ? ws : rs[lr + k]);
      }
    }
    if (COLS) {
      float f[4][8];
#pragma unroll
      for (int k = 0; k < 4; ++k) unpack8(v[step][k], f[k]);
#pragma unroll
      for (int j = 0; j < 8; ++j)  // rows lr .. lr + 3 of column 8 ci + j: one dword (lr % 4 == 0, 132 % 4 == 0)
        *reinterpret_cast<uint32_t*>(tile + (8 * ci + j) * kTileLds + lr) =
            cvt4_e4m3(fp8_train_q(f[0][j], sc[j]), fp8_train_q(f[1][j], sc[j]), fp8_train_q(f[2][j], sc[j]), fp8_train_q(f[3][j], sc[j]));
    }
  }
  if (COLS) {
    __syncthreads();
    // 128 columns x 8 pieces of 16 bytes (= 16 rows each); R % 128 == 0: every piece lies inside
    for (int p = threadIdx.x; p < kTile * 8; p += kThreads) {
      const int col = p >> 3, part = p & 7;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(tile + col * kTileLds + part * 16);
      *reinterpret_cast<u32x4*>(q_col_t + (c0 + col) * R + r0 + part * 16) = u32x4{src[0], src[1], src[2], src[3]};
    }
  }
}

// ---- the weight gradient ------------------------------------------------------------------------------------------------------------------
using namespace wgrad_stage;  // the stage layout, wgrad_issue, wgrad_frag

struct BlockWgradArgs {
  const uint8_t* g;    // e4m3 [N][M]
  const float* g_inv;  // [M/128][N]
  const uint8_t* x;    // e4m3 [K][M]
  const float* x_inv;  // [M/128][K]
  uint16_t* out;       // bf16 [N][K]
  int M, N, K;
};

// the lane's scales of token block `step`: g_inv of its rows 16 i + 4 kq + {0..3} (one 16-byte load each), x_inv of its columns 16 j + l % 16
__device__ __forceinline__ void wgrad_scales(const float* g_row, const float* x_col, int step, int N, int K, f32x4 (&gs)[4], float (&xs)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    gs[i] = *reinterpret_cast<const f32x4*>(g_row + (size_t)step * N + 16 * i);
    xs[i] = x_col[(size_t)step * K + 16 * i];
  }
}

__global__ __launch_bounds__(256) void fp8_block_wgrad_kernel(BlockWgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4;
  const int n0 = blockIdx.y * 128, k0 = blockIdx.x * 128;
  const int wn = (wave >> 1) * 64, wk = (wave & 1) * 64;
  const int steps = p.M >> 7;
  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)p.g, 0, p.N * p.M, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.K * p.M, 0x00020000);
  // M, N and K are multiples of 128: every row, token and scale index of a tile lies inside
  const float* g_row = p.g_inv + n0 + wn + 4 * kq;
  const float* x_col = p.x_inv + k0 + wk + (lane & 15);
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 gs[4];
  float xs[4];
  wgrad_scales(g_row, x_col, 0, p.N, p.K, gs, xs);
  wgrad_issue(rg, rx, smem, n0, k0, 0, p.M, p.N, p.K, wave, lane);
  for (int step = 0; step < steps; ++step) {
    char* cur = smem + (step & 1) * kStage;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage `step` has landed for every wave; every wave is done with the other stage
    f32x4 ngs[4];
    float nxs[4];
    if (step + 1 < steps) {
      wgrad_issue(rg, rx, smem + ((step + 1) & 1) * kStage, n0, k0, step + 1, p.M, p.N, p.K, wave, lane);
      wgrad_scales(g_row, x_col, step + 1, p.N, p.K, ngs, nxs);
    }
    u32x4 xf0[4], xf1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wgrad_frag(cur + kOpBytes, wk + 16 * j + (lane & 15), kq, xf0[j], xf1[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 g0, g1;
      wgrad_frag(cur, wn + 16 * i + (lane & 15), kq, g0, g1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 prod = mfma8_k128<false>(g0, g1, xf0[j], xf1[j], f32x4{0.f, 0.f, 0.f, 0.f});
        acc[i][j] = fp8_block_acc(acc[i][j], prod, gs[i], xs[j]);
      }
    }
    if (step + 1 < steps) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        gs[i] = ngs[i];
        xs[i] = nxs[i];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = k0 + wk + 16 * j + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + 16 * i + 4 * kq + r;
        p.out[(size_t)n * p.K + k] = f32_to_bf16_bits(fp8_block_out(acc[i][j][r]));
      }
  }
}

// ---- the grouped weight gradient (ao_fp8_block_grouped_mm_wgrad) --------------------------------------------------------------------------
//   out[e][n][k] = bf16(sum over the token blocks mb that meet group e = [offs[e-1], offs[e]), ascending, of (p * g_inv[mb][n]) * x_inv[mb][k]),
//   p = the block's tokens INSIDE the group as one scaled MFMA onto a zero accumulator.
// The grid (tiles of K, tiles of N, E), the clamp of offs to [0, M] and the register masks of a step's foreign tokens are fp8_wgrad_kernel's
// (fp8_grouped_train_kernels.hip); the stages, the chain and the scale prefetch are fp8_block_wgrad_kernel's.  The block scales sit on the
// GLOBAL 128-token grid (the casts know no groups), so a block that two groups share is multiplied twice, each time with the other group's
// codes zeroed.  An empty group runs no step and stores zeros; no split along the tokens.
struct BlockGroupedWgradArgs {
  const uint8_t* g;     // e4m3 [N][M]
  const float* g_inv;   // [M/128][N]
  const uint8_t* x;     // e4m3 [K][M]
  const float* x_inv;   // [M/128][K]
  const int32_t* offs;  // [E] cumulative ends; null: one group [0, M)
  uint16_t* out;        // bf16 [E][N][K]
  int M, N, K;
};

__global__ __launch_bounds__(256, 2) void fp8_block_grouped_wgrad_kernel(BlockGroupedWgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4;
  const int e = blockIdx.z;
  const int n0 = blockIdx.y * 128, k0 = blockIdx.x * 128;
  const int wn = (wave >> 1) * 64, wk = (wave & 1) * 64;
  // the group's tokens, clamped to the matrix; a range that runs backwards is an empty group
  const int start = p.offs != nullptr ? min(max(e > 0 ? p.offs[e - 1] : 0, 0), p.M) : 0;
  const int end = p.offs != nullptr ? min(max(p.offs[e], 0), p.M) : p.M;
  const int s0 = start >> 7, s1 = end > start ? (end + 127) >> 7 : s0;  // end <= M and M % 128 == 0: s1 <= M / 128
  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)p.g, 0, p.N * p.M, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.K * p.M, 0x00020000);
  // M, N and K are multiples of 128: every row, token and scale index of a tile lies inside
  const float* g_row = p.g_inv + n0 + wn + 4 * kq;
  const float* x_col = p.x_inv + k0 + wk + (lane & 15);
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 gs[4];
  float xs[4];
  if (s0 < s1) {
    wgrad_scales(g_row, x_col, s0, p.N, p.K, gs, xs);
    wgrad_issue(rg, rx, smem + (s0 & 1) * kStage, n0, k0, s0, p.M, p.N, p.K, wave, lane);
  }
  for (int step = s0; step < s1; ++step) {
    char* cur = smem + (step & 1) * kStage;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage `step` has landed for every wave; every wave is done with the other stage
    f32x4 ngs[4];
    float nxs[4];
    if (step + 1 < s1) {
      wgrad_issue(rg, rx, smem + ((step + 1) & 1) * kStage, n0, k0, step + 1, p.M, p.N, p.K, wave, lane);
      wgrad_scales(g_row, x_col, step + 1, p.N, p.K, ngs, nxs);
    }
    // a step that reaches outside the group: the lane's two 16-token pieces keep the group's own tokens only
    const bool edge = step * 128 < start || step * 128 + 128 > end;  // wave-uniform
    u32x4 mk0, mk1;
    if (edge) {
      mk0 = token_mask(step * 128 + 16 * kq, start, end);
      mk1 = token_mask(step * 128 + 64 + 16 * kq, start, end);
    }
    u32x4 xf0[4], xf1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wgrad_frag(cur + kOpBytes, wk + 16 * j + (lane & 15), kq, xf0[j], xf1[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 g0, g1;
      wgrad_frag(cur, wn + 16 * i + (lane & 15), kq, g0, g1);
      if (edge) {
        g0 &= mk0;
        g1 &= mk1;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 prod = mfma8_k128<false>(g0, g1, xf0[j], xf1[j], f32x4{0.f, 0.f, 0.f, 0.f});
        acc[i][j] = fp8_block_acc(acc[i][j], prod, gs[i], xs[j]);
      }
    }
    if (step + 1 < s1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        gs[i] = ngs[i];
        xs[i] = nxs[i];
      }
    }
  }
  uint16_t* out = p.out + (size_t)e * p.N * p.K;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = k0 + wk + 16 * j + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + 16 * i + 4 * kq + r;
        out[(size_t)n * p.K + k] = f32_to_bf16_bits(fp8_block_out(acc[i][j][r]));
      }
  }
}

bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the shape of a cast: both extents multiples of 128 where the direction needs it, and a grid that one launch holds
int check_cast(const char* fn, int64_t R, int64_t C, bool whole_rows) {
  AO_REQUIRE(R >= 0 && C >= 0 && C % 128 == 0, "%s: bad shape R=%lld C=%lld (C must be a multiple of 128)", fn, (long long)R, (long long)C);
  AO_REQUIRE(!whole_rows || R % 128 == 0, "%s: R=%lld must be a multiple of 128 for 128-row blocks", fn, (long long)R);
  AO_REQUIRE((R + kTile - 1) / kTile <= 65535 && C / kTile < (1ll << 31), "%s: R=%lld C=%lld too large for one launch", fn, (long long)R,
             (long long)C);
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_fp8_block_train_cast(const uint16_t* x, uint8_t* q_row, float* inv_row, uint8_t* q_col_t, float* inv_col, int64_t R,
                                       int64_t C, void* stream) {
  const bool rows = q_row != nullptr || inv_row != nullptr, cols = q_col_t != nullptr || inv_col != nullptr;
  if (int rc = check_cast(__func__, R, C, cols)) return rc;
  if (R == 0 || C == 0) return AO_OK;
  AO_REQUIRE(rows || cols, "%s: neither (q_row, inv_row) nor (q_col_t, inv_col) given", __func__);
  AO_REQUIRE_PTR(x);
  if (rows) {
    AO_REQUIRE_PTR(q_row);
    AO_REQUIRE_PTR(inv_row);
  }
  if (cols) {
    AO_REQUIRE_PTR(q_col_t);
    AO_REQUIRE_PTR(inv_col);
  }
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(q_row, 16) && aligned_to(q_col_t, 16) && aligned_to(inv_row, 4) && aligned_to(inv_col, 4),
             "%s: x and the codes must be 16-byte, the scales 4-byte aligned", __func__);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(C / kTile), (unsigned)((R + kTile - 1) / kTile)), block(kThreads);
  if (rows && cols) ao::launch(fp8_block_train_cast_kernel<true, true, false>, grid, block, 0, s, x, q_row, inv_row, q_col_t, inv_col, R, C);
  else if (rows) ao::launch(fp8_block_train_cast_kernel<true, false, false>, grid, block, 0, s, x, q_row, inv_row, q_col_t, inv_col, R, C);
  else ao::launch(fp8_block_train_cast_kernel<false, true, false>, grid, block, 0, s, x, q_row, inv_row, q_col_t, inv_col, R, C);
  AO_LAUNCH_CHECK("fp8_block_train_cast_kernel launch");
  return AO_OK;
}

extern "C" int ao_fp8_block_train_cast_weight(const uint16_t* w, uint8_t* q, float* inv, uint8_t* q_t, float* inv_t, int64_t N, int64_t K,
                                              void* stream) {
  const bool plain = q != nullptr || inv != nullptr, trans = q_t != nullptr || inv_t != nullptr;
  if (int rc = check_cast(__func__, N, K, true)) return rc;
  if (N == 0 || K == 0) return AO_OK;
  AO_REQUIRE(plain || trans, "%s: neither (q, inv) nor (q_t, inv_t) given", __func__);
  AO_REQUIRE_PTR(w);
  if (plain) {
    AO_REQUIRE_PTR(q);
    AO_REQUIRE_PTR(inv);
  }
  if (trans) {
    AO_REQUIRE_PTR(q_t);
    AO_REQUIRE_PTR(inv_t);
  }
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(q, 16) && aligned_to(q_t, 16) && aligned_to(inv, 4) && aligned_to(inv_t, 4),
             "%s: w and the codes must be 16-byte, the scales 4-byte aligned", __func__);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(K / kTile), (unsigned)(N / kTile)), block(kThreads);
  if (plain && trans) ao::launch(fp8_block_train_cast_kernel<true, true, true>, grid, block, 0, s, w, q, inv, q_t, inv_t, N, K);
  else if (plain) ao::launch(fp8_block_train_cast_kernel<true, false, true>, grid, block, 0, s, w, q, inv, q_t, inv_t, N, K);
  else ao::launch(fp8_block_train_cast_kernel<false, true, true>, grid, block, 0, s, w, q, inv, q_t, inv_t, N, K);
  AO_LAUNCH_CHECK("fp8_block_train_cast_kernel (weight) launch");
  return AO_OK;
}

extern "C" int ao_fp8_block_train_cast_weight_3d(const uint16_t* w, uint8_t* q, float* inv, uint8_t* q_t, float* inv_t, int64_t E, int64_t N,
                                                 int64_t K, void* stream) {
  const bool plain = q != nullptr || inv != nullptr, trans = q_t != nullptr || inv_t != nullptr;
  AO_REQUIRE(E >= 0 && N >= 0 && K >= 0, "%s: bad shape E=%lld N=%lld K=%lld", __func__, (long long)E, (long long)N, (long long)K);
  AO_REQUIRE(N % 128 == 0 && K % 128 == 0, "%s: N=%lld and K=%lld must be multiples of 128 (a 128 x 128 block lies in one expert)", __func__,
             (long long)N, (long long)K);
  if (E == 0 || N == 0 || K == 0) return AO_OK;
  AO_REQUIRE(E <= 65535, "%s: E=%lld must be at most 65535", __func__, (long long)E);
  AO_REQUIRE(E * (N / kTile) <= 65535 && K / kTile < (1ll << 31), "%s: E=%lld N=%lld K=%lld too large for one launch (at most 65535 tiles of 128 rows)",
             __func__, (long long)E, (long long)N, (long long)K);
  AO_REQUIRE(plain || trans, "%s: neither (q, inv) nor (q_t, inv_t) given", __func__);
  AO_REQUIRE_PTR(w);
  if (plain) {
    AO_REQUIRE_PTR(q);
    AO_REQUIRE_PTR(inv);
  }
  if (trans) {
    AO_REQUIRE_PTR(q_t);
    AO_REQUIRE_PTR(inv_t);
  }
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(q, 16) && aligned_to(q_t, 16) && aligned_to(inv, 4) && aligned_to(inv_t, 4),
             "%s: w and the codes must be 16-byte, the scales 4-byte aligned", __func__);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(K / kTile), (unsigned)(N / kTile), (unsigned)E), block(kThreads);
  if (plain && trans) ao::launch(fp8_block_train_cast_kernel<true, true, true, true>, grid, block, 0, s, w, q, inv, q_t, inv_t, N, K);
  else if (plain) ao::launch(fp8_block_train_cast_kernel<true, false, true, true>, grid, block, 0, s, w, q, inv, q_t, inv_t, N, K);
  else ao::launch(fp8_block_train_cast_kernel<false, true, true, true>, grid, block, 0, s, w, q, inv, q_t, inv_t, N, K);
  AO_LAUNCH_CHECK("fp8_block_train_cast_kernel (3-D weight) launch");
  return AO_OK;
}

extern "C" int ao_fp8_block_grouped_mm_wgrad(const uint8_t* g_t, const float* g_inv, const uint8_t* x_t, const float* x_inv, const int32_t* offs,
                                             uint16_t* out, int64_t M, int64_t N, int64_t K, int64_t E, void* stream) {
  AO_REQUIRE(M >= 0 && N > 0 && K > 0, "%s: bad shape M=%lld N=%lld K=%lld", __func__, (long long)M, (long long)N, (long long)K);
  AO_REQUIRE(M % 128 == 0 && N % 128 == 0 && K % 128 == 0, "%s: M=%lld, N=%lld and K=%lld must be multiples of 128", __func__, (long long)M,
             (long long)N, (long long)K);
  AO_REQUIRE(E >= 1 && E <= 65535, "%s: E=%lld must be in 1..65535 (the grid's z extent)", __func__, (long long)E);
  AO_REQUIRE(offs != nullptr || E == 1, "%s: without offs there is one group of every token, got E=%lld", __func__, (long long)E);
  AO_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31) && N * M < (1ll << 31) && K * M < (1ll << 31) && N / 128 <= 65535,
             "%s: M=%lld N=%lld K=%lld: the sizes and both operands' byte counts must be below 2^31", __func__, (long long)M, (long long)N,
             (long long)K);
  AO_REQUIRE_PTR(out);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (M == 0) {
    const hipError_t rc = hipMemsetAsync(out, 0, (size_t)E * N * K * sizeof(uint16_t), st);
    if (rc != hipSuccess) return hip_failed(rc, "hipMemsetAsync(fp8_block_grouped_mm_wgrad)");
    return AO_OK;
  }
  AO_REQUIRE_PTR(g_t);
  AO_REQUIRE_PTR(g_inv);
  AO_REQUIRE_PTR(x_t);
  AO_REQUIRE_PTR(x_inv);
  AO_REQUIRE(aligned_to(g_t, 16) && aligned_to(x_t, 16) && aligned_to(g_inv, 16) && aligned_to(x_inv, 4) && aligned_to(out, 2) &&
                 aligned_to(offs, 4),
             "%s: the codes and g_inv must be 16-byte, x_inv and offs 4-byte and out 2-byte aligned", __func__);
  constexpr size_t smem = 2 * kStage;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(fp8_block_grouped_wgrad_kernel), smem,
                                  "hipFuncSetAttribute(fp8_block_grouped_wgrad_kernel)"))
    return rc;
  const BlockGroupedWgradArgs args{g_t, g_inv, x_t, x_inv, offs, out, (int)M, (int)N, (int)K};
  ao::launch(fp8_block_grouped_wgrad_kernel, dim3((unsigned)(K / 128), (unsigned)(N / 128), (unsigned)E), dim3(256), smem, st, args);
  AO_LAUNCH_CHECK("fp8_block_grouped_wgrad_kernel launch");
  return AO_OK;
}

extern "C" int ao_fp8_block_mm_wgrad(const uint8_t* g_t, const float* g_inv, const uint8_t* x_t, const float* x_inv, uint16_t* out, int64_t M,
                                     int64_t N, int64_t K, void* stream) {
  AO_REQUIRE(M >= 0 && N > 0 && K > 0, "%s: bad shape M=%lld N=%lld K=%lld", __func__, (long long)M, (long long)N, (long long)K);
  AO_REQUIRE(M % 128 == 0 && N % 128 == 0 && K % 128 == 0, "%s: M=%lld, N=%lld and K=%lld must be multiples of 128", __func__, (long long)M,
             (long long)N, (long long)K);
  AO_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31) && N * M < (1ll << 31) && K * M < (1ll << 31) && N / 128 <= 65535,
             "%s: M=%lld N=%lld K=%lld: the sizes and both operands' byte counts must be below 2^31", __func__, (long long)M, (long long)N,
             (long long)K);
  AO_REQUIRE_PTR(out);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (M == 0) {
    const hipError_t rc = hipMemsetAsync(out, 0, (size_t)N * K * sizeof(uint16_t), st);
    if (rc != hipSuccess) return hip_failed(rc, "hipMemsetAsync(fp8_block_mm_wgrad)");
    return AO_OK;
  }
  AO_REQUIRE_PTR(g_t);
  AO_REQUIRE_PTR(g_inv);
  AO_REQUIRE_PTR(x_t);
  AO_REQUIRE_PTR(x_inv);
  AO_REQUIRE(aligned_to(g_t, 16) && aligned_to(x_t, 16) && aligned_to(g_inv, 16) && aligned_to(x_inv, 4) && aligned_to(out, 2),
             "%s: the codes and g_inv must be 16-byte, x_inv 4-byte and out 2-byte aligned", __func__);
  constexpr size_t smem = 2 * kStage;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(fp8_block_wgrad_kernel), smem, "hipFuncSetAttribute(fp8_block_wgrad_kernel)"))
    return rc;
  const BlockWgradArgs args{g_t, g_inv, x_t, x_inv, out, (int)M, (int)N, (int)K};
  ao::launch(fp8_block_wgrad_kernel, dim3((unsigned)(K / 128), (unsigned)(N / 128)), dim3(256), smem, st, args);
  AO_LAUNCH_CHECK("fp8_block_wgrad_kernel launch");
  return AO_OK;
}
