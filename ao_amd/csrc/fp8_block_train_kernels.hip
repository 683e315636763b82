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
// The weight gradient (kernels.py:320-379, triton_fp8_gemm_1x128_128x1): out[n][k] = bf16(sum over token blocks mb, ascending, of
// (p * g_inv[mb][n]) * x_inv[mb][k]), p = the block's 128 tokens as ONE scaled MFMA onto a zero accumulator.  fp8_block_grouped_wgrad_kernel
// is the weight-gradient frame (wgrad_frame.h) with fp8_block_acc per k step; the scale vectors of step mb + 1 (128 contiguous floats
// each per tile) are loaded into registers while step mb multiplies.  A lane's rows 4 kq + r take g_inv as fp8_block_acc's a_s; its
// column is fixed per j, so x_inv is fp8_block_acc's b_s, one value per lane.
//
// The routed experts (torchao/prototype/moe_training/blockwise_fp8/grouped_mm.py:98-265): the weight cast over a stack of
// experts is the same cast kernel with the expert in blockIdx.z (ao_fp8_block_train_cast_weight_3d), and ao_fp8_block_grouped_mm_wgrad is
// the weight gradient per token group on the same column casts of all tokens; the dense ao_fp8_block_mm_wgrad is its one group of every
// token.
#include "common.h"
#include "quant_math.h"
#include "stream_blocks.h"
#include "fp8_train_tile.h"
#include "wgrad_frame.h"

namespace ao {
namespace {

using namespace fp8_train_tile;  // the constants and the helpers of the tile walk

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
  __shared__ __attribute__((aligned(16))) uint8_t tile[COLS ? kTileLdsBytes : 16];
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
  load_tile<false>(x, r0, c, R, C, wave, g, v);
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
  if (kColMax) reduce_cols(cm, cred[wave], ci, g);
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
    if (COLS) stage_cols_t(tile, v[step], sc, ci, lr);
  }
  if (COLS) {
    __syncthreads();
    // R % 128 == 0: every piece lies inside
    flush_cols_t<false>(tile, c0, r0, C, R, [&](int64_t gc, int64_t gr) { return q_col_t + gc * R + gr; });
  }
}

// ---- the weight gradient (ao_fp8_block_grouped_mm_wgrad, ao_fp8_block_mm_wgrad) -------------------------------------------------------------
//   out[e][n][k] = bf16(sum over the token blocks mb that meet group e = [offs[e-1], offs[e]), ascending, of (p * g_inv[mb][n]) * x_inv[mb][k]),
//   p = the block's tokens INSIDE the group as one scaled MFMA onto a zero accumulator.
// The block scales sit on the GLOBAL 128-token grid (the casts know no groups), as the frame's k steps do, so a block that two groups share
// is multiplied twice, each time with the other group's codes zeroed.
using namespace wgrad_frame;

struct BlockWgradArgs {
  const uint8_t* g;     // e4m3 [N][M]
  const float* g_inv;   // [M/128][N]
  const uint8_t* x;     // e4m3 [K][M]
  const float* x_inv;   // [M/128][K]
  const int32_t* offs;  // [E] cumulative ends; null: one group [0, M)
  uint16_t* out;        // bf16 [E][N][K]
  int M, N, K;
};

// M, N and K are multiples of 128: every row, token and scale index of a tile lies inside
struct BlockPolicy {
  struct Scales {
    f32x4 g[4];  // g_inv of the lane's rows 16 i + 4 kq + {0..3}: one 16-byte load each
    float x[4];  // x_inv of its columns 16 j + l % 16
  };
  const float *g_row, *x_col;
  const BlockWgradArgs& p;
  // (the tile's part joins the pointer first, in scalar registers)
  __device__ __forceinline__ BlockPolicy(const BlockWgradArgs& p, const Lane& t, int)
      : g_row(p.g_inv + t.n0 + t.wn + 4 * t.kq), x_col(p.x_inv + t.k0 + t.wk + t.l16), p(p) {}
  __device__ __forceinline__ void load(int step, Scales& s) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s.g[i] = *reinterpret_cast<const f32x4*>(g_row + (size_t)step * p.N + 16 * i);
      s.x[i] = x_col[(size_t)step * p.K + 16 * i];
    }
  }
  __device__ __forceinline__ f32x4 mac(f32x4 acc, u32x4 g0, u32x4 g1, u32x4 x0, u32x4 x1, const Scales& s, int i, int j) const {
    const f32x4 prod = mfma8_k128<false>(g0, g1, x0, x1, f32x4{0.f, 0.f, 0.f, 0.f});
    return fp8_block_acc(acc, prod, s.g[i], s.x[j]);
  }
  __device__ __forceinline__ void store(uint16_t* out, const f32x4 (&acc)[4][4], const Lane& t) const {
    wgrad_store<false>(out, t, p.N, p.K, [&](int i, int j, int r, int, int) { return fp8_block_out(acc[i][j][r]); });
  }
};

__global__ __launch_bounds__(256, 2) void fp8_block_grouped_wgrad_kernel(BlockWgradArgs p) {
  wgrad_tile<BlockPolicy>(p);
}

// both weight-gradient entries; dense: no offs, one group of every token
int block_wgrad(const char* fn, const uint8_t* g_t, const float* g_inv, const uint8_t* x_t, const float* x_inv, const int32_t* offs, uint16_t* out,
                int64_t M, int64_t N, int64_t K, int64_t E, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  bool launch;
  if (int rc = check_entry(Entry{fn, "M", 128, 128, true}, g_t, x_t, offs, out, M, N, K, E, st, &launch)) return rc;
  if (!launch) return AO_OK;
  AO_REQUIRE_PTR_FN(fn, g_inv);
  AO_REQUIRE_PTR_FN(fn, x_inv);
  AO_REQUIRE(aligned_to(g_inv, 16) && aligned_to(x_inv, 4) && aligned_to(out, 2) && aligned_to(offs, 4),
             "%s: g_inv must be 16-byte, x_inv and offs 4-byte and out 2-byte aligned", fn);
  const BlockWgradArgs args{g_t, g_inv, x_t, x_inv, offs, out, (int)M, (int)N, (int)K};
  return launch_frame(fp8_block_grouped_wgrad_kernel, "fp8_block_grouped_wgrad_kernel", args, N, K, E, st);
}

// the shape of a cast: both extents multiples of 128 where the direction needs it, and a grid that one launch holds
int check_cast(const char* fn, int64_t R, int64_t C, bool whole_rows) {
  AO_REQUIRE(R >= 0 && C >= 0 && C % 128 == 0, "%s: bad shape R=%lld C=%lld (C must be a multiple of 128)", fn, (long long)R, (long long)C);
  AO_REQUIRE(!whole_rows || R % 128 == 0, "%s: R=%lld must be a multiple of 128 for 128-row blocks", fn, (long long)R);
  AO_REQUIRE((R + kTile - 1) / kTile <= 65535 && C / kTile < (1ll << 31), "%s: R=%lld C=%lld too large for one launch", fn, (long long)R,
             (long long)C);
  return AO_OK;
}

// What the three cast entries share once the shape is checked and not empty: each layout is asked for by its pair of pointers (the plain
// pair is the kernel's ROWS, the transposed one its COLS), half a pair is a null pointer; the alignment; the instantiation that writes
// what is asked for.
template <bool WEIGHT, bool BATCHED>
int launch_cast(const char* fn, const uint16_t* in, uint8_t* q, float* inv, uint8_t* q_t, float* inv_t, int64_t R, int64_t C, dim3 grid,
                void* stream) {
  const bool plain = q != nullptr || inv != nullptr, trans = q_t != nullptr || inv_t != nullptr;
  AO_REQUIRE(plain || trans, "%s: neither the plain pair (codes, reciprocals) nor the transposed one given", fn);
  AO_REQUIRE_PTR_FN(fn, in);
  if (plain) {
    AO_REQUIRE_PTR_FN(fn, q);
    AO_REQUIRE_PTR_FN(fn, inv);
  }
  if (trans) {
    AO_REQUIRE_PTR_FN(fn, q_t);
    AO_REQUIRE_PTR_FN(fn, inv_t);
  }
  AO_REQUIRE(aligned_to(in, 16) && aligned_to(q, 16) && aligned_to(q_t, 16) && aligned_to(inv, 4) && aligned_to(inv_t, 4),
             "%s: the input and the codes must be 16-byte, the scales 4-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(kThreads);
  if (plain && trans) ao::launch(fp8_block_train_cast_kernel<true, true, WEIGHT, BATCHED>, grid, block, 0, s, in, q, inv, q_t, inv_t, R, C);
  else if (plain) ao::launch(fp8_block_train_cast_kernel<true, false, WEIGHT, BATCHED>, grid, block, 0, s, in, q, inv, q_t, inv_t, R, C);
  else ao::launch(fp8_block_train_cast_kernel<false, true, WEIGHT, BATCHED>, grid, block, 0, s, in, q, inv, q_t, inv_t, R, C);
  AO_LAUNCH_CHECK("fp8_block_train_cast_kernel launch");
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_fp8_block_train_cast(const uint16_t* x, uint8_t* q_row, float* inv_row, uint8_t* q_col_t, float* inv_col, int64_t R,
                                       int64_t C, void* stream) {
  const bool cols = q_col_t != nullptr || inv_col != nullptr;
  if (int rc = check_cast(__func__, R, C, cols)) return rc;
  if (R == 0 || C == 0) return AO_OK;
  const dim3 grid((unsigned)(C / kTile), (unsigned)((R + kTile - 1) / kTile));
  return launch_cast<false, false>(__func__, x, q_row, inv_row, q_col_t, inv_col, R, C, grid, stream);
}

extern "C" int ao_fp8_block_train_cast_weight(const uint16_t* w, uint8_t* q, float* inv, uint8_t* q_t, float* inv_t, int64_t N, int64_t K,
                                              void* stream) {
  if (int rc = check_cast(__func__, N, K, true)) return rc;
  if (N == 0 || K == 0) return AO_OK;
  const dim3 grid((unsigned)(K / kTile), (unsigned)(N / kTile));
  return launch_cast<true, false>(__func__, w, q, inv, q_t, inv_t, N, K, grid, stream);
}

extern "C" int ao_fp8_block_train_cast_weight_3d(const uint16_t* w, uint8_t* q, float* inv, uint8_t* q_t, float* inv_t, int64_t E, int64_t N,
                                                 int64_t K, void* stream) {
  AO_REQUIRE(E >= 0 && N >= 0 && K >= 0, "%s: bad shape E=%lld N=%lld K=%lld", __func__, (long long)E, (long long)N, (long long)K);
  AO_REQUIRE(N % 128 == 0 && K % 128 == 0, "%s: N=%lld and K=%lld must be multiples of 128 (a 128 x 128 block lies in one expert)", __func__,
             (long long)N, (long long)K);
  if (E == 0 || N == 0 || K == 0) return AO_OK;
  AO_REQUIRE(E <= 65535, "%s: E=%lld must be at most 65535", __func__, (long long)E);
  AO_REQUIRE(E * (N / kTile) <= 65535 && K / kTile < (1ll << 31), "%s: E=%lld N=%lld K=%lld too large for one launch (at most 65535 tiles of 128 rows)",
             __func__, (long long)E, (long long)N, (long long)K);
  const dim3 grid((unsigned)(K / kTile), (unsigned)(N / kTile), (unsigned)E);
  return launch_cast<true, true>(__func__, w, q, inv, q_t, inv_t, N, K, grid, stream);
}

extern "C" int ao_fp8_block_grouped_mm_wgrad(const uint8_t* g_t, const float* g_inv, const uint8_t* x_t, const float* x_inv, const int32_t* offs,
                                             uint16_t* out, int64_t M, int64_t N, int64_t K, int64_t E, void* stream) {
  return block_wgrad(__func__, g_t, g_inv, x_t, x_inv, offs, out, M, N, K, E, stream);
}

extern "C" int ao_fp8_block_mm_wgrad(const uint8_t* g_t, const float* g_inv, const uint8_t* x_t, const float* x_inv, uint16_t* out, int64_t M,
                                     int64_t N, int64_t K, void* stream) {
  return block_wgrad(__func__, g_t, g_inv, x_t, x_inv, nullptr, out, M, N, K, 1, stream);
}
