// NVFP4 training of the MoE grouped GEMM for gfx950: the per-group casts, the per-expert weight cast and the weight-gradient GEMM whose
// contraction runs along the jagged token dimension.
//
// Replaces, of torchao's prototype/moe_training/nvfp4_training: triton_group_rht_amax (group_hadamard_amax_triton.py),
// triton_group_rht_quantize_row_col (group_rht_quantize_row_col_triton.py), triton_group_weight_amax (group_weight_amax_triton.py),
// triton_group_weight_quantize_2d (group_quantize_2d_triton.py) and the weight-gradient F.scaled_grouped_mm of _NVFP4GroupedMM
// (nvfp4_grouped_mm.py:315-326), which run on sm100 only.  Each grouped cast there is "a launch optimization, not a different recipe":
// every group is cast like a dense tensor under its own amaxes, so the arithmetic is quant_math.h's ("NVFP4 training") and the tile walk
// is nvfp4_train_tile.h's, instantiated GROUPED.  Scales stay ROW-MAJOR, so a group needs 16-row alignment (the transform's runs and the
// 1 x 16 blocks along the tokens), not the 128 of the reference's swizzled scales.
//
// nvfp4_train_group_amax_kernel: the dense amax kernel's unit -- 16 rows x 2 adjacent columns a thread, both transforms in registers -- but
//   a WAVE takes a contiguous range of (run of 16 rows, 64 column pairs) tasks, so its group only ever moves forward: it keeps one running
//   pair of maxima and spills it (wave max, one atomic max a value on the non-negative bit patterns) when the group changes and at the end.
// nvfp4_train_weight_amax_3d_kernel: grid (parts, E), max|w[e]| by 16-byte pieces, one atomic a wave.
// nvfp4_wgrad_kernel: the weight gradient,
//     out[e][n][k] = bf16( (sum over the tokens m of group e of dq(g_t)[n][m] dq(x_t)[k][m]) (pg[e] px[e]) ),
//   grid (tiles of K, tiles of N, E), 128 x 128 output tiles, four waves of 64 x 64, 4 x 4 accumulators of v_mfma_f32_16x16x32_bf16 a wave:
//   wgrad_frame.h's grid, lane placement and store walk.  Its stage does not fit: that frame moves 128 code BYTES a row and step by
//   buffer_load ... lds in 16-byte pieces and hands the MFMA the bytes as they lie; here a 64-token step of a row is 32 bytes of codes and 4
//   scale bytes, a row of codes is only 8-byte aligned (16 | M_total), the scale bytes have no alignment at all, and a fragment must be
//   DECODED on its way to the MFMA.  So the kernel has its own stage:
//     stage  128 rows x 40 bytes an operand (32 code bytes, 4 scale bytes, 4 of padding), two stages.  Thread t fetches, for row t / 2 of
//            each operand, the two 16-token blocks 2 (t % 2) and 2 (t % 2) + 1 of the step: 8 bytes of codes and a scale byte each, into
//            registers under the MFMAs of the step before, then into the other stage -- one barrier a step.
//     walk   the steps cover the GLOBAL 16-token grid from start / 16 in runs of four blocks, so every 8-byte load is aligned whatever the
//            offsets are, and only a group's LAST step can reach foreign tokens.
//     decode lane (l16, kq) of a fragment takes the WHOLE block kq of its row: one ds_read_b64, one scale byte, nvfp4_block16 -- code x
//            block scale is exact in bf16 -- gives the operands of two MFMAs (k slots 8 kq .. 8 kq + 7 hold tokens 16 kq + 8 h ...; both
//            operands use the same placement, which is all the sum needs).  No shuffles, one scale a block.
//   Foreign tokens -- a neighbour group's inside the last step, or past M_total -- enter with scale byte 0 in BOTH operands (their codes are
//   loaded if they exist, zero otherwise): e2m1 has no NaN or Inf, so code x 0 is 0 and a neighbour's NaN scale byte cannot leak.  Rows past
//   N / K are staged as zero and not stored.  An empty group stores zeros.  No split along the tokens, no atomics: a launch is reproducible.
#include "common.h"
#include "nvfp4_train_tile.h"
#include "quant_math.h"
#include "wgrad_frame.h"

#include <algorithm>

namespace ao {
namespace {

using namespace nvfp4_train;

// ---- the per-group amax pair ------------------------------------------------------------------------------------------------------------
__global__ void nvfp4_train_clear_kernel(uint32_t* out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = 0u;
}

__device__ __forceinline__ void group_amax_spill(uint32_t* out, int g, float mc, float mr) {
  mc = wave_max(mc);
  mr = wave_max(mr);
  if ((threadIdx.x & 63) == 0) {
    if (mc > 0.f) atomicMax(out + 2 * g, f32_to_bits(mc));  // (cleared to 0: nothing to add otherwise)
    if (mr > 0.f) atomicMax(out + 2 * g + 1, f32_to_bits(mr));
  }
}

__global__ __launch_bounds__(kThreads) void nvfp4_train_group_amax_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ offs,
                                                                          int64_t M, int64_t N, int E, uint32_t sign_mask, int want_rht,
                                                                          uint32_t* out) {
  const int64_t half = N >> 1, cw = (half + 63) >> 6, tasks = (M >> 4) * cw;
  const int64_t waves = (int64_t)gridDim.x * (kThreads / 64), wave = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const int64_t t0 = tasks * wave / waves, t1 = tasks * (wave + 1) / waves;  // (tasks < 2^40, waves <= 4096)
  const int lane = threadIdx.x & 63;
  const uint32_t* px = reinterpret_cast<const uint32_t*>(x);
  int cur = -1;
  float mr = 0.f, mc = 0.f;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t mb = t / cw, c2 = (t - mb * cw) * 64 + lane;
    const int g = group_of_row(offs, E, mb * 16);  // wave-uniform
    if (g != cur) {
      if (cur >= 0 && cur < E) group_amax_spill(out, cur, mc, mr);
      cur = g;
      mr = mc = 0.f;
    }
    if (g >= E || c2 >= half) continue;  // a capacity run reaches no reduction
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
  if (cur >= 0 && cur < E) group_amax_spill(out, cur, mc, mr);
}

// ---- max|w[e]| ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nvfp4_train_weight_amax_3d_kernel(const uint16_t* __restrict__ w, int64_t pieces, uint32_t* out) {
  const u32x4* pw = reinterpret_cast<const u32x4*>(w) + (size_t)blockIdx.y * (size_t)pieces;
  float m = 0.f;
  bool has_nan = false;  // (NaN is outside the contract, as in ao_nvfp4_train_amax)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pieces; i += (int64_t)gridDim.x * 256) m = fmaxf(m, amax8(pw[i], has_nan));
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(out + blockIdx.y, f32_to_bits(m));
}

// ---- the weight-gradient GEMM -------------------------------------------------------------------------------------------------------------
constexpr int kRow = 40;               // bytes a staged row: 32 of codes, 4 scale bytes, 4 of padding (8-byte aligned blocks)
constexpr int kOp = 128 * kRow;        // one operand of a stage
constexpr int kStage = 2 * kOp;        // g then x

struct WgradArgs {
  const uint8_t* g;    // codes [N][M/2]
  const uint8_t* gs;   // e4m3 [N][M/16]
  const uint8_t* x;    // codes [K][M/2]
  const uint8_t* xs;   // e4m3 [K][M/16]
  const float* pg;     // [E]
  const float* px;     // [E]
  const int32_t* offs; // [E] or null: one group of every token
  uint16_t* out;       // bf16 [E][N][K]
  int M, N, K;
};

__device__ __forceinline__ f32x4 mfma_bf16(const u32x4& a, const u32x4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// one decoded fragment of a step: the lane's block of 16 tokens of row r as the operands of the step's two MFMAs
__device__ __forceinline__ void wgrad_decode(const char* op, int r, int kq, u32x4& h0, u32x4& h1) {
  const u32x2 q = *reinterpret_cast<const u32x2*>(op + r * kRow + 8 * kq);
  const uint32_t s8 = *reinterpret_cast<const uint8_t*>(op + r * kRow + 32 + kq);
  nvfp4_block16(q, e4m3_byte_to_f32(s8), h0, h1);
}

__global__ __launch_bounds__(256) void nvfp4_wgrad_kernel(WgradArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kStage];
  const unsigned tid = threadIdx.x;
  __builtin_assume(tid < 256u);
  const int lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
  const int e = blockIdx.z;
  const wgrad_frame::Lane t{lane & 15, kq, (int)blockIdx.y * 128, (int)blockIdx.x * 128, (wave >> 1) * 64, (wave & 1) * 64};
  // the group's tokens in blocks of 16, clamped to the matrix; a range that runs backwards is an empty group
  const int mb = p.M >> 4;
  const int b0 = p.offs != nullptr ? min(max((e > 0 ? p.offs[e - 1] : 0) >> 4, 0), mb) : 0;
  const int b1 = p.offs != nullptr ? min(max(p.offs[e] >> 4, 0), mb) : mb;
  const int steps = b1 > b0 ? (b1 - b0 + 3) >> 2 : 0;
  // what this thread stages: row sr of g and of x, blocks sc and sc + 1 of the step
  const int sr = tid >> 1, sc = 2 * (tid & 1);
  const bool g_ok = t.n0 + sr < p.N, x_ok = t.k0 + sr < p.K;
  const uint8_t* gq = p.g + (size_t)(g_ok ? t.n0 + sr : 0) * (size_t)(p.M >> 1);
  const uint8_t* gs = p.gs + (size_t)(g_ok ? t.n0 + sr : 0) * (size_t)mb;
  const uint8_t* xq = p.x + (size_t)(x_ok ? t.k0 + sr : 0) * (size_t)(p.M >> 1);
  const uint8_t* xs = p.xs + (size_t)(x_ok ? t.k0 + sr : 0) * (size_t)mb;
  u32x2 fq[2][2];   // [operand][block]
  uint32_t fs[2];   // [operand]: the two scale bytes
  auto fetch = [&](int step) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int blk = b0 + 4 * step + sc + c;
      const bool own = blk < b1;  // (b1 <= M / 16: a block of the group exists)
      const u32x2 z = {0u, 0u};
      fq[0][c] = (own && g_ok) ? *reinterpret_cast<const u32x2*>(gq + (size_t)blk * 8) : z;
      fq[1][c] = (own && x_ok) ? *reinterpret_cast<const u32x2*>(xq + (size_t)blk * 8) : z;
      const uint32_t sg = (own && g_ok) ? (uint32_t)gs[blk] : 0u, sx = (own && x_ok) ? (uint32_t)xs[blk] : 0u;
      fs[0] = c == 0 ? sg : fs[0] | (sg << 8);
      fs[1] = c == 0 ? sx : fs[1] | (sx << 8);
    }
  };
  auto park = [&](char* stage) {
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      char* row = stage + o * kOp + sr * kRow;
      *reinterpret_cast<u32x2*>(row + 8 * sc) = fq[o][0];
      *reinterpret_cast<u32x2*>(row + 8 * sc + 8) = fq[o][1];
      *reinterpret_cast<uint16_t*>(row + 32 + sc) = (uint16_t)fs[o];
    }
  };
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (steps > 0) {
    fetch(0);
    park(smem);
  }
  for (int step = 0; step < steps; ++step) {
    const char* cur = smem + (step & 1) * kStage;
    __syncthreads();  // stage `step` is parked by every thread; every wave is done with the other stage
    const bool more = step + 1 < steps;
    if (more) fetch(step + 1);  // in flight under the MFMAs
    u32x4 xf0[4], xf1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wgrad_decode(cur + kOp, t.wk + 16 * j + t.l16, kq, xf0[j], xf1[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 g0, g1;
      wgrad_decode(cur, t.wn + 16 * i + t.l16, kq, g0, g1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[i][j] = mfma_bf16(g0, xf0[j], acc[i][j]);
        acc[i][j] = mfma_bf16(g1, xf1[j], acc[i][j]);
      }
    }
    if (more) park(smem + ((step + 1) & 1) * kStage);
  }
  // (an empty group stores zeros whatever its scales hold)
  bool has_P = false;
  const float P = steps > 0 ? nvfp4_P(p.pg + e, p.px + e, has_P) : 0.f;  // the fp32 product of the two scales
  const bool empty = steps == 0;
  wgrad_frame::wgrad_store<true>(p.out + (size_t)e * p.N * p.K, t, p.N, p.K,
                                 [&](int i, int j, int r, int, int) { return empty ? 0.f : nvfp4_scaled_mm_out(acc[i][j][r], P); });
}

int check_sign_mask(const char* fn, uint32_t sign_mask) {
  AO_REQUIRE(sign_mask < (1u << 16), "%s: sign_mask must be a 16-bit mask, got 0x%x", fn, sign_mask);
  return AO_OK;
}

int check_experts(const char* fn, int64_t E) {
  AO_REQUIRE(E >= 1 && E <= 65535, "%s: E=%lld must be in [1, 65535]", fn, (long long)E);
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_nvfp4_train_group_amax(const uint16_t* x, const int32_t* offs, float* out, int64_t M_total, int64_t N, int64_t E,
                                         uint32_t sign_mask, int want_rht, void* stream) {
  if (int rc = check_mn(__func__, M_total, N)) return rc;
  if (int rc = check_experts(__func__, E)) return rc;
  if (int rc = check_sign_mask(__func__, sign_mask)) return rc;
  AO_REQUIRE_PTR(offs);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(out, 4) && aligned_to(offs, 4), "%s: out and offs must be 4-byte aligned", __func__);
  if (M_total > 0) {
    AO_REQUIRE_PTR(x);
    AO_REQUIRE(aligned_to(x, 16), "%s: x must be 16-byte aligned", __func__);
  }
  // every check is above: nothing is launched for a call that is refused
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* bits = reinterpret_cast<uint32_t*>(out);
  ao::launch(nvfp4_train_clear_kernel, dim3((unsigned)((2 * E + 255) / 256)), dim3(256), 0, s, bits, (int)(2 * E));
  if (M_total > 0) {
    const int64_t tasks = (M_total / 16) * ((N / 2 + 63) / 64);
    const int64_t grid = std::min<int64_t>((tasks + 3) / 4, 1024);
    ao::launch(nvfp4_train_group_amax_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, x, offs, M_total, N, (int)E, sign_mask, want_rht, bits);
  }
  AO_LAUNCH_CHECK("nvfp4_train_group_amax kernels launch");
  return AO_OK;
}

extern "C" int ao_nvfp4_train_quantize_row_col_grouped(const uint16_t* x, const float* amax, const int32_t* offs, uint32_t sign_mask,
                                                       const int64_t* sr_seed, const int64_t* col_offset, const int64_t* row_offset,
                                                       uint8_t* col_q, uint8_t* col_s, uint8_t* row_q, uint8_t* row_s, int64_t M_total, int64_t N,
                                                       int64_t E, void* stream) {
  if (int rc = check_mn(__func__, M_total, N)) return rc;
  if (int rc = check_experts(__func__, E)) return rc;
  if (int rc = check_sign_mask(__func__, sign_mask)) return rc;
  AO_REQUIRE((col_q == nullptr) == (col_s == nullptr) && (row_q == nullptr) == (row_s == nullptr),
             "%s: an output's codes and scales are given together or both null", __func__);
  AO_REQUIRE(col_q != nullptr || row_q != nullptr, "%s: both outputs are null", __func__);
  AO_REQUIRE_PTR(amax);
  AO_REQUIRE_PTR(offs);
  if (sr_seed != nullptr) {
    if (col_q != nullptr) AO_REQUIRE_PTR(col_offset);
    if (row_q != nullptr) AO_REQUIRE_PTR(row_offset);
  }
  if (M_total == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(col_q, 8) && aligned_to(row_q, 8) && aligned_to(amax, 4) && aligned_to(offs, 4) &&
                 aligned_to(sr_seed, 8) && aligned_to(col_offset, 8) && aligned_to(row_offset, 8),
             "%s: x must be 16-byte, the codes, the seed and the offsets 8-byte, amax and offs 4-byte aligned", __func__);
  const TrainCastArgs a{x, amax, amax + 1, sign_mask, sr_seed, col_offset, row_offset, col_q, col_s, row_q, row_s, M_total, N, offs, (int)E};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return sr_seed != nullptr ? launch_cast<false, true, true>(a, 1, st) : launch_cast<false, false, true>(a, 1, st);
}

extern "C" int ao_nvfp4_train_weight_amax_3d(const uint16_t* w, float* out, int64_t E, int64_t N, int64_t K, void* stream) {
  if (int rc = check_mn(__func__, N, K)) return rc;
  if (int rc = check_experts(__func__, E)) return rc;
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(out, 4), "%s: out must be 4-byte aligned", __func__);
  if (N > 0) {
    AO_REQUIRE_PTR(w);
    AO_REQUIRE(aligned_to(w, 16), "%s: w must be 16-byte aligned", __func__);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* bits = reinterpret_cast<uint32_t*>(out);
  ao::launch(nvfp4_train_clear_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, bits, (int)E);
  if (N > 0) {
    const int64_t pieces = N * K / 8;
    const int64_t parts = std::max<int64_t>(1, std::min<int64_t>({(pieces + 255) / 256, 1024, (16384 + E - 1) / E}));
    ao::launch(nvfp4_train_weight_amax_3d_kernel, dim3((unsigned)parts, (unsigned)E), dim3(256), 0, s, w, pieces, bits);
  }
  AO_LAUNCH_CHECK("nvfp4_train_weight_amax_3d kernels launch");
  return AO_OK;
}

extern "C" int ao_nvfp4_train_quantize_weight_3d(const uint16_t* w, const float* amax, uint8_t* q, uint8_t* s, uint8_t* qt, uint8_t* st, int64_t E,
                                                 int64_t N, int64_t K, void* stream) {
  if (int rc = check_mn(__func__, N, K)) return rc;
  if (int rc = check_experts(__func__, E)) return rc;
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
  return launch_cast<true, false, true>(a, E, static_cast<hipStream_t>(stream));
}

extern "C" int ao_nvfp4_grouped_mm_wgrad(const uint8_t* g_t, const uint8_t* g_scale, const uint8_t* x_t, const uint8_t* x_scale, const float* pg,
                                         const float* px, const int32_t* offs, uint16_t* out, int64_t M_total, int64_t N, int64_t K, int64_t E,
                                         void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  bool run = false;
  // (the frame's alignment check asks 16 bytes of the codes; the kernel reads 8 at a time)
  if (int rc = wgrad_frame::check_entry({__func__, "M_total", 16, 16, true}, g_t, x_t, offs, out, M_total, N, K, E, st, &run)) return rc;
  if (!run) return AO_OK;
  AO_REQUIRE_PTR(g_scale);
  AO_REQUIRE_PTR(x_scale);
  AO_REQUIRE_PTR(pg);
  AO_REQUIRE_PTR(px);
  AO_REQUIRE(aligned_to(pg, 4) && aligned_to(px, 4) && aligned_to(offs, 4) && aligned_to(out, 2),
             "%s: the per-expert scales and offs must be 4-byte, out 2-byte aligned", __func__);
  const WgradArgs a{g_t, g_scale, x_t, x_scale, pg, px, offs, out, (int)M_total, (int)N, (int)K};
  ao::launch(nvfp4_wgrad_kernel, dim3((unsigned)((K + 127) / 128), (unsigned)((N + 127) / 128), (unsigned)E), dim3(256), 0, st, a);
  AO_LAUNCH_CHECK("nvfp4_wgrad_kernel launch");
  return AO_OK;
}
