// float8 rowwise training of the MoE grouped GEMM for gfx950: the casts that follow token groups, the transposing cast of a 3-D weight and
// the 2-D x 2-D grouped GEMM of the weight gradient.  The arithmetic of the casts is that of fp8_train_kernels.hip, stated once in
// quant_math.h (fp8_train_scale, fp8_train_q), their tile walk in fp8_train_tile.h; the GEMM is the weight-gradient frame (wgrad_frame.h).
//
// Reference (torchao 0.19.0 snapshot, prototype/moe_training):
//   jagged cast : kernels/jagged_float8_scales.py:221-252, utils.py:20-86 (torch_to_float8_per_group_colwise): one scale per column and
//                 token group, the amax over the group's rows
//   3-D cast    : kernels/float8_rowwise.py, utils.py:156-189 (torch_to_3d_rowwise_float8_transpose_rhs): one scale per (expert, column),
//                 the codes stored transposed
//   wgrad GEMM  : fp8_grouped_mm.py:282-319 (torch._scaled_grouped_mm on the two jagged casts, 2-D x 2-D with offsets)
//
// Both casts are ONE walk over 16-row slabs in which every slab belongs to one "group" whose [C] scale vector it uses:
//   jagged : x [R][C], group e = rows [offs[e-1], offs[e]); every end is a multiple of 16, so a slab lies in one group; rows at or past
//            offs[E-1] belong to none and get code 0.  The group of a slab is found by a binary search of offs (an upper bound): for ANY
//            int32 contents the index stays in [0, E], offs values are compared and never used as an index.
//   batched: w [E][R][C] seen as [E R][C], group e = rows [e R, (e + 1) R) (R % 16 == 0); the codes of expert e leave as [C][R] at e C R.
// Three launches behind a memset: column maxima per group (atomic max into the [E][C] buffer that becomes `s`), scales and reciprocals in
// place, codes.  A wave owns one slab per step (fp8_train_tile.h), so the group index is wave-uniform.
#include "common.h"
#include "quant_math.h"
#include "fp8_train_tile.h"
#include "stream_blocks.h"
#include "wgrad_frame.h"

namespace ao {
namespace {

using namespace fp8_train_tile;
using namespace wgrad_frame;

constexpr int kSlabs = kTile / 16;

// The group of the 16-row slab that starts at row r: E for "none" (a row past the matrix or past the last group).
template <bool BATCHED>
__device__ __forceinline__ int slab_group(const int32_t* __restrict__ offs, int E, int64_t r, int64_t rows, int64_t rows_per) {
  if (r >= rows) return E;
  if (BATCHED) return (int)(r / rows_per);
  int lo = 0, hi = E;  // the first e with offs[e] > r
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)offs[mid] > r) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// ---- amax: max |x| of every column over each group's rows, merged into the zeroed [E][C] buffer by an unsigned atomic max ------------------
// The slabs of a tile merge in LDS first: a run of slabs of one group costs one atomic per column.
template <bool BATCHED>
__global__ __launch_bounds__(kThreads) void fp8_group_amax_cols_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ offs,
                                                                       float* __restrict__ amax, int64_t rows, int64_t C, int64_t rows_per,
                                                                       int E) {
  __shared__ float cred[kSlabs][kTile];
  __shared__ int sgrp[kSlabs];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.y * kTile, c = (int64_t)blockIdx.x * kTile + 8 * ci;
  u32x4 v[2][4];
  load_tile<true>(x, r0, c, rows, C, wave, g, v);
#pragma unroll
  for (int step = 0; step < 2; ++step) {
    const int slab = step * 4 + wave;
    float cm[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float f[8];
      unpack8(v[step][k], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) cm[j] = fmaxf(cm[j], fabsf(f[j]));
    }
    reduce_cols(cm, cred[slab], ci, g);
    if (lane == 0) sgrp[slab] = slab_group<BATCHED>(offs, E, r0 + 16 * slab, rows, rows_per);
  }
  __syncthreads();
  const int64_t gc = (int64_t)blockIdx.x * kTile + threadIdx.x;
  if (threadIdx.x < kTile && gc < C) {
    const int t = threadIdx.x;
    int e = sgrp[0];
    float m = cred[0][t];
#pragma unroll
    for (int s = 1; s <= kSlabs; ++s) {
      const int en = s < kSlabs ? sgrp[s] : -1;
      if (en == e) {
        m = fmaxf(m, cred[s][t]);
      } else {
        if (e < E) atomicMax(reinterpret_cast<unsigned int*>(amax + (int64_t)e * C + gc), f32_to_bits(m));
        if (s < kSlabs) {
          e = en;
          m = cred[s][t];
        }
      }
    }
  }
}

// ---- scales: amax -> scale in place, and its reciprocal (an empty group's amax is the memset's zero: the scale of 1e-12) --------------------
__global__ __launch_bounds__(kThreads) void fp8_group_scale_kernel(float* __restrict__ s, float* __restrict__ inv_s, int pow2, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) {
    const float sc = fp8_train_scale(s[i], pow2 != 0);
    s[i] = sc;
    inv_s[i] = 1.0f / sc;
  }
}

// ---- cast: the codes, transposed through LDS as in fp8_train_cast_kernel<false, true>; a slab of no group leaves as zeros -----------------
// q_t: jagged [C][rows]; batched [E][C][rows_per].
template <bool BATCHED>
__global__ __launch_bounds__(kThreads) void fp8_group_cast_cols_t_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ offs,
                                                                         const float* __restrict__ s, uint8_t* __restrict__ q_t,
                                                                         int64_t rows, int64_t C, int64_t rows_per, int E) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTileLdsBytes];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.y * kTile, c0 = (int64_t)blockIdx.x * kTile, c = c0 + 8 * ci;
  u32x4 v[2][4];
  load_tile<true>(x, r0, c, rows, C, wave, g, v);
#pragma unroll
  for (int step = 0; step < 2; ++step) {
    const int lr = tile_row(step, wave, g);
    const int e = __builtin_amdgcn_readfirstlane(slab_group<BATCHED>(offs, E, r0 + 16 * (step * 4 + wave), rows, rows_per));
    const bool live = e < E && c < C;  // C % 16 == 0: a lane's 8 columns are inside together
    float sc[8];
    if (live) {
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(s + (int64_t)e * C + c), s1 = *reinterpret_cast<const f32x4*>(s + (int64_t)e * C + c + 4);
      sc[0] = s0.x; sc[1] = s0.y; sc[2] = s0.z; sc[3] = s0.w;
      sc[4] = s1.x; sc[5] = s1.y; sc[6] = s1.z; sc[7] = s1.w;
    }
    stage_cols_t(tile, v[step], sc, ci, lr, live);
  }
  __syncthreads();
  // a piece is one slab: (batched, rows_per % 16 == 0) it lies inside one expert
  flush_cols_t<true>(tile, c0, r0, C, rows, [&](int64_t gc, int64_t gr) {
    return BATCHED ? q_t + (gr / rows_per) * C * rows_per + gc * rows_per + gr % rows_per : q_t + gc * rows + gr;
  });
}

// rows = the rows walked (R, or E R batched); the grid's y extent carries 65535 tiles of 128 rows
template <bool BATCHED>
int group_cast(const uint16_t* x, const int32_t* offs, uint8_t* q_t, float* s, float* inv_s, int pow2, int64_t rows,
               int64_t C, int64_t rows_per, int64_t E, hipStream_t st) {
  hipError_t rc = hipMemsetAsync(s, 0, (size_t)E * C * sizeof(float), st);
  if (rc != hipSuccess) return hip_failed(rc, "hipMemsetAsync(fp8 group amax)");
  const dim3 grid((unsigned)((C + kTile - 1) / kTile), (unsigned)((rows + kTile - 1) / kTile)), block(kThreads);
  ao::launch(fp8_group_amax_cols_kernel<BATCHED>, grid, block, 0, st, x, offs, s, rows, C, rows_per, (int)E);
  AO_LAUNCH_CHECK("fp8_group_amax_cols_kernel launch");
  ao::launch(fp8_group_scale_kernel, dim3((unsigned)((E * C + kThreads - 1) / kThreads)), block, 0, st, s, inv_s, pow2, E * C);
  AO_LAUNCH_CHECK("fp8_group_scale_kernel launch");
  ao::launch(fp8_group_cast_cols_t_kernel<BATCHED>, grid, block, 0, st, x, offs, (const float*)s, q_t, rows, C, rows_per, (int)E);
  AO_LAUNCH_CHECK("fp8_group_cast_cols_t_kernel launch");
  return AO_OK;
}

// ---- the grouped weight gradient -----------------------------------------------------------------------------------------------------------
//   out[e][n][k] = bf16( (sum_{m in [offs[e-1], offs[e])} g_t[n][m] x_t[k][m]) * g_inv[e][n] * x_inv[e][k] )
// The weight-gradient frame (wgrad_frame.h) with nothing per k step: the MFMA's scales are 2^0 and the two rowwise reciprocal scales of
// the expert meet the fp32 sum in the epilogue (epilogue8<false>, quant_math.h).  Any offsets.
struct Fp8WgradArgs {
  const uint8_t* g;    // e4m3 [N][M]
  const float* g_inv;  // [E][N]
  const uint8_t* x;    // e4m3 [K][M]
  const float* x_inv;  // [E][K]
  const int32_t* offs; // [E] cumulative ends; null: one group [0, M)
  uint16_t* out;       // bf16 [E][N][K]
  int M, N, K;
};

struct RowwisePolicy {
  struct Scales {};
  const Fp8WgradArgs& p;
  const float *gi, *xi;  // the expert's reciprocals
  __device__ __forceinline__ RowwisePolicy(const Fp8WgradArgs& p, const Lane&, int e)
      : p(p), gi(p.g_inv + (size_t)e * p.N), xi(p.x_inv + (size_t)e * p.K) {}
  __device__ __forceinline__ void load(int, Scales&) const {}
  __device__ __forceinline__ f32x4 mac(f32x4 acc, u32x4 g0, u32x4 g1, u32x4 x0, u32x4 x1, const Scales&, int, int) const {
    return mfma8_k128<false, AO_MX_FMT_E4M3>(g0, g1, x0, x1, acc);
  }
  __device__ __forceinline__ void store(uint16_t* out, const f32x4 (&acc)[4][4], const Lane& t) const {
    // the lane's 16 row scales first: a store to out may alias g_inv for all the compiler knows, and would have it load them again
    float sg[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = t.nrow() + 16 * i + r;
        sg[i][r] = n < p.N ? gi[n] : 0.f;
      }
    float sx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sx[j] = t.kcol() + 16 * j < p.K ? xi[t.kcol() + 16 * j] : 0.f;
    wgrad_store<true>(out, t, p.N, p.K, [&](int i, int j, int r, int, int) { return epilogue8<false>(acc[i][j][r], sg[i][r], sx[j]); });
  }
};

__global__ __launch_bounds__(256) void fp8_wgrad_kernel(Fp8WgradArgs p) {
  wgrad_tile<RowwisePolicy>(p);
}

constexpr int64_t kMaxGroups = 65535;  // the wgrad grid's z extent; the casts' binary search has no limit of its own

int check_cast_shape(const char* fn, int64_t R, int64_t C, int64_t E, int64_t rows) {
  AO_REQUIRE(R >= 0 && C >= 0 && E > 0, "%s: bad shape R=%lld C=%lld E=%lld", fn, (long long)R, (long long)C, (long long)E);
  AO_REQUIRE(R % 16 == 0, "%s: R=%lld must be a multiple of 16 (a 16-row slab lies in one group; the rows are the GEMM's K)", fn, (long long)R);
  AO_REQUIRE(C % 16 == 0, "%s: C=%lld must be a multiple of 16", fn, (long long)C);
  AO_REQUIRE(E <= kMaxGroups, "%s: E=%lld must be at most %lld", fn, (long long)E, (long long)kMaxGroups);
  AO_REQUIRE((rows + kTile - 1) / kTile <= 65535 && (C + kTile - 1) / kTile < (1ll << 31) && E * C < (1ll << 40),
             "%s: %lld rows x C=%lld (E=%lld) too large for one launch (at most 65535 tiles of 128 rows)", fn, (long long)rows, (long long)C,
             (long long)E);
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_fp8_train_quantize_group_colwise_t(const uint16_t* x, const int32_t* offs, uint8_t* q_t, float* s, float* inv_s, int pow2,
                                                     int64_t R, int64_t C, int64_t E, void* stream) {
  if (int rc = check_cast_shape(__func__, R, C, E, R)) return rc;
  if (R == 0 || C == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(offs);
  AO_REQUIRE_PTR(q_t);
  AO_REQUIRE_PTR(s);
  AO_REQUIRE_PTR(inv_s);
  AO_REQUIRE(aligned16(x) && aligned16(q_t) && aligned16(s), "%s: x, q_t and s must be 16-byte aligned", __func__);
  return group_cast<false>(x, offs, q_t, s, inv_s, pow2, R, C, R, E, (hipStream_t)stream);
}

extern "C" int ao_fp8_train_quantize_colwise_t_3d(const uint16_t* w, uint8_t* q_t, float* s, float* inv_s, int pow2, int64_t E, int64_t R,
                                                  int64_t C, void* stream) {
  AO_REQUIRE(E >= 0, "%s: bad shape E=%lld", __func__, (long long)E);
  if (int rc = check_cast_shape(__func__, R, C, E > 0 ? E : 1, E * R)) return rc;
  if (E == 0 || R == 0 || C == 0) return AO_OK;
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(q_t);
  AO_REQUIRE_PTR(s);
  AO_REQUIRE_PTR(inv_s);
  AO_REQUIRE(aligned16(w) && aligned16(q_t) && aligned16(s), "%s: w, q_t and s must be 16-byte aligned", __func__);
  return group_cast<true>(w, nullptr, q_t, s, inv_s, pow2, E * R, C, R, E, (hipStream_t)stream);
}

extern "C" int ao_fp8_grouped_mm_wgrad(const uint8_t* g_t, const float* g_inv, const uint8_t* x_t, const float* x_inv, const int32_t* offs,
                                       uint16_t* out, int64_t M_total, int64_t N, int64_t K, int64_t E, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  bool launch;
  if (int rc = check_entry(Entry{__func__, "M_total", 16, 16, true}, g_t, x_t, offs, out, M_total, N, K, E, st, &launch)) return rc;
  if (!launch) return AO_OK;
  AO_REQUIRE_PTR(g_inv);
  AO_REQUIRE_PTR(x_inv);
  const Fp8WgradArgs args{g_t, g_inv, x_t, x_inv, offs, out, (int)M_total, (int)N, (int)K};
  return launch_frame(fp8_wgrad_kernel, "fp8_wgrad_kernel", args, N, K, E, st);
}
