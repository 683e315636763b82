// NVFP4 linears for gfx950: e2m1 codes, one e4m3 scale per 1 x 16 block along K, an optional fp32 per-tensor scale.
//
// Replaces, of torchao's NVFP4Tensor (prototype/mx_formats/nvfp4_tensor.py): the cast (nvfp4_quantize :772-854 with
// per_tensor_amax_to_scale :756-769 and the dynamic torch.max(torch.abs(x)) of :605-607), the weight-only linear (:593-596: dequantize,
// then F.linear) and the NVFP4 x NVFP4 GEMM (_addmm_nvfp4_dispatch :487-578: torch._scaled_mm on sm100).  The arithmetic contracts are
// stated once, in quant_math.h ("NVFP4").
//
// CDNA4's scaled MFMA takes one E8M0 scale per 32 k, so an e4m3 scale per 16 k does not fit it.  code x block scale is exact in bf16
// (2 + 4 significand bits, exponent far inside the range), so both GEMMs decode their 4-bit operands to bf16 in registers
// (nvfp4_block16) and run v_mfma_f32_16x16x32_bf16 with fp32 accumulation: the products and the accumulation of a native FP4 unit, in
// another summation order, at the bf16 MFMA's rate.  The MFMA sums over k in whatever order its lanes hold it, so a lane takes WHOLE
// blocks: one scale a block and no shuffles.
//
// Two forms, one route (nvfp4_route: this family's shape check, seams and forced form over the plans of
// two_form_route.h) read by the launches and by ao_nvfp4_linear_route / _kernel_name; KIND 0 the weight-only linear, 1 codes x codes:
//   nvfp4_stream_kernel: the weight is streamed once, 0.5625 bytes a weight.  A workgroup owns 16 columns and splits K over its waves in
//     runs of 128-k steps; lane (column l & 15, group kq) takes the 32 k at 32 kq of a step -- 16 bytes of codes, two scale bytes -- and
//     feeds four MFMAs; a wave requests a chunk of four steps ahead of the chunk it multiplies, nontemporal.  The activation (bf16, or
//     codes decoded the same way) is read inside the multiply.  The partial tiles meet in LDS in wave order.
//   nvfp4_tile_kernel: 64 x 64 output tiles, four waves of 32 x 32, both operands staged in LDS as bf16 -- a block decoded ONCE, by the
//     thread that stages it -- with the next k step's global loads in flight under the MFMAs.  A first cut: correct for every M, ragged
//     N and K; not tuned.
//
// The grouped GEMM for MoE experts (ao_nvfp4_grouped_mm; the reference: NVFP4Tensor's aten._grouped_mm :709-753 over mslk /
// sm100, or the bf16 emulation of prototype/moe_training/nvfp4_grouped_mm.py:62-116) applies the same chains, without a bias, per token
// group [offs[e-1], offs[e]) against expert e: the GROUPED instantiations of the two kernels above -- the same bodies -- routed on the mean
// group size (nvfp4_grouped_route), with the per-group amax and cast next to the dense ones.
#include "common.h"
#include "quant_math.h"
#include "two_form_route.h"

#include <algorithm>

namespace ao {
namespace {

constexpr int kKindWo = AO_NVFP4_KIND_WEIGHT_ONLY;
constexpr int kKindDyn = AO_NVFP4_KIND_DYNAMIC;

// ---- the route ------------------------------------------------------------------------------------------------------------------
// Chosen on the Llama-3-8B five shapes (profiles/nvfp4_linear.jsonl: its "fit" lines, tools/bench_nvfp4_linear.py --sweep, both forms
// forced at M = 1 .. 256, weights from HBM, the five shapes summed over every swept M per candidate seam): the streaming form up to these
// rows, the LDS-tiled form beyond.  Weight-only: 3353 us at 64, 3321 at 65, 3351 at 96, rising on both sides (3456 at 48, 3427 at 128) --
// flat between 64 and 96; the constant takes 64, the last row count the stream form serves with ONE grid row.  Codes x codes: the minimum
// is 64 (3791 us; 3813 at 65, 3925 at 48).  (At 64 rows the five shapes take 250 us streamed, 352 us tiled (weight-only), 246 / 380
// (codes x codes); at 128 rows 432 / 356 and 425 / 392.)
constexpr int kStreamMaxRowsWo = 64;
constexpr int kStreamMaxRowsDyn = 64;

thread_local int g_form = 0;  // ao_nvfp4_linear_set_form: 0 the product route, 1 stream, 2 tile

bool nvfp4_shape_ok(int kind, int64_t M, int64_t N, int64_t K) {
  if (kind != kKindWo && kind != kKindDyn) return false;
  if (M < 0 || N < 1 || K < 16 || K % 16 != 0) return false;
  // K + 1024 below 2^31: the kernels walk k in 32-bit steps of up to 128 past the last one of a chunk
  if (M >= (1ll << 31) || N >= (1ll << 31) || K > (1ll << 31) - 1024) return false;
  return M * K < (1ll << 31) && N * K < (1ll << 31) && M * N < (1ll << 40);
}

// kernel 1: nvfp4_stream_kernel, 2: nvfp4_tile_kernel (64 x 64 tiles)
TwoFormRoute nvfp4_route(int kind, int64_t M, int64_t N, int64_t K) {
  if (!nvfp4_shape_ok(kind, M, N, K)) return TwoFormRoute{};
  const int seam = kind == kKindWo ? kStreamMaxRowsWo : kStreamMaxRowsDyn;
  TwoFormRoute r = two_form_route(g_form != 0 ? g_form : (M <= seam ? 1 : 2), M, N, K, 64);
  r.grid_y = std::max(r.grid_y, 1);  // (the tiled form reports one grid row at M = 0 -- a forced form only; never launched)
  return r;
}

struct Nvfp4Args {
  const uint16_t* x;       // bf16 [M][K] (weight-only)
  const uint8_t* a;        // codes [M][K/2] (codes x codes)
  const uint8_t* a_scale;  // e4m3 [M][K/16]
  const uint8_t* b;        // codes [N][K/2]
  const uint8_t* b_scale;  // e4m3 [N][K/16]
  const float* pa;         // per-tensor scale of the activation codes, or null
  const float* pb;         // per-tensor scale of the weight, or null
  const uint16_t* bias;    // bf16 [N] or null
  uint16_t* out;           // bf16 [M][N]
  int M, N, K;
  // grouped (MoE experts) only: M is M_total, b / b_scale hold E experts, pa / pb one scale an expert, no bias
  const int32_t* offs;     // [E] cumulative group ends, or null (dense)
  int E;
  // codes x codes only: the epilogue of ao_nvfp4_scaled_mm, out = bf16(acc (pa pb)) rounded once (nvfp4_scaled_mm_out), not nvfp4_mm_out's chain
  int scaled_mm;
};

// Token group e = rows [offs[e-1], offs[e]) (offs[-1] = 0).  The kernels only read offs: a group's bounds are clamped to [0, M_total] (a
// bad offs cannot address outside the activation or out) and a non-increasing pair is an empty group.
__device__ __forceinline__ int clamp_row(int r, int M_total) { return r < 0 ? 0 : (r > M_total ? M_total : r); }
__device__ __forceinline__ void group_bounds(const int32_t* offs, int e, int M_total, int& row_begin, int& row_end) {
  row_begin = clamp_row(e > 0 ? offs[e - 1] : 0, M_total);
  row_end = clamp_row(offs[e], M_total);
}

__device__ __forceinline__ f32x4 mfma_bf16(const u32x4& a, const u32x4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// The 32 codes (16 bytes) at k0 of a row of codes and their two scale bytes (low byte: the block at k0).  k32: K is a multiple of 32 --
// rows of codes are 16-byte aligned and hold whole pairs of blocks; otherwise the row's last block stands alone and rows are 8-byte
// aligned, so the halves are loaded on their own.  A block past K reads the row's first block (zeroed by the caller).
template <bool NT>
__device__ __forceinline__ void load_blocks(const uint8_t* row, const uint8_t* srow, int k0, int K, bool k32, u32x4& q, uint32_t& s) {
  const bool v0 = k0 < K, v1 = k0 + 16 < K;
  if (k32) {
    const u32x4* pq = reinterpret_cast<const u32x4*>(row + (v0 ? k0 >> 1 : 0));
    q = NT ? __builtin_nontemporal_load(pq) : *pq;
    s = *reinterpret_cast<const uint16_t*>(srow + (v0 ? k0 >> 4 : 0));
  } else {
    const u32x2* p0 = reinterpret_cast<const u32x2*>(row + (v0 ? k0 >> 1 : 0));
    const u32x2* p1 = reinterpret_cast<const u32x2*>(row + (v1 ? (k0 >> 1) + 8 : 0));
    const u32x2 lo = NT ? __builtin_nontemporal_load(p0) : *p0, hi = NT ? __builtin_nontemporal_load(p1) : *p1;
    q = u32x4{lo.x, lo.y, hi.x, hi.y};
    s = (uint32_t)srow[v0 ? k0 >> 4 : 0] | ((uint32_t)srow[v1 ? (k0 >> 4) + 1 : 0] << 8);
  }
}

// 32 codes -> 32 bf16 (four MFMA operands); blocks past K are zero
__device__ __forceinline__ void decode_blocks(const u32x4& q, uint32_t s, bool has_p, float p, bool v0, bool v1, u32x4 (&w)[4]) {
  const u32x4 z = {0u, 0u, 0u, 0u};
  w[0] = w[1] = w[2] = w[3] = z;
  if (v0) nvfp4_block16(u32x2{q.x, q.y}, nvfp4_scale32(s & 0xffu, has_p, p), w[0], w[1]);
  if (v1) nvfp4_block16(u32x2{q.z, q.w}, nvfp4_scale32((s >> 8) & 0xffu, has_p, p), w[2], w[3]);
}

// ---- streaming form -------------------------------------------------------------------------------------------------------------
constexpr int kChunk = 4;  // 128-k steps a wave requests at once

// ONE body, two instantiations per (KIND, MT, WAVES):
//   GROUPED false, "nvfp4_stream_kernel": the dense linear; blockIdx.y is the workgroup's block of 16 MT rows.
//   GROUPED true, "nvfp4_grouped_stream_kernel": grid (ceil(N / 16), E); blockIdx.y is the expert, and the workgroup walks its group's rows
//     16 MT at a time: a pass is the dense body (the weight comes from L2 from the second pass on), with a barrier before the next pass
//     reuses the meeting buffer.  pb[e] is folded into the decode (weight-only); P_e = pa[e] pb[e] is applied in the epilogue.
template <int KIND, int MT, int WAVES, bool GROUPED>
__global__ __launch_bounds__(64 * WAVES) void nvfp4_stream_kernel(Nvfp4Args p) {
  __shared__ f32x4 red[WAVES][MT][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kq = lane >> 4;
  const int n = blockIdx.x * 16 + (lane & 15);
  int m0 = blockIdx.y * 16 * MT, row_end = p.M;
  if constexpr (GROUPED) {
    group_bounds(p.offs, blockIdx.y, p.M, m0, row_end);
    if (row_end <= m0) return;  // an empty group: the whole workgroup leaves, before any barrier
    // the expert's base in 64 bits: the whole b may pass 2^31 elements
    p.b += (size_t)blockIdx.y * p.N * (p.K >> 1);
    p.b_scale += (size_t)blockIdx.y * p.N * (p.K >> 4);
    if (p.pa != nullptr) p.pa += blockIdx.y;
    if (p.pb != nullptr) p.pb += blockIdx.y;
  }
  const int ksteps = (p.K + 127) >> 7;
  const int ks0 = (ksteps * wave) / WAVES, ks1 = (ksteps * (wave + 1)) / WAVES;
  const int kb = p.K >> 4;
  const bool k32 = (p.K & 31) == 0;
  // columns past N read the last row (never stored)
  const uint8_t* wrow = p.b + (size_t)min(n, p.N - 1) * (p.K >> 1);
  const uint8_t* wsrow = p.b_scale + (size_t)min(n, p.N - 1) * kb;
  int kq32 = 32 * kq;
  // the weight-only linear folds the weight's per-tensor scale into the weights (dequantize); codes x codes applies P after the sum
  const bool has_pw = KIND == kKindWo && p.pb != nullptr;
  const float pw = has_pw ? *p.pb : 1.f;
  struct Stage {
    u32x4 q;
    uint32_t s;
  };
  auto issue = [&](Stage (&st)[kChunk], int step) {
#pragma unroll
    for (int d = 0; d < kChunk; ++d) load_blocks<true>(wrow, wsrow, (step + d) * 128 + kq32, p.K, k32, st[d].q, st[d].s);
    __builtin_amdgcn_sched_barrier(0);  // every request of the chunk is out before anything waits
  };
  for (;; m0 += 16 * MT) {  // (dense: one pass)
    // (grouped: a pass recomputes its addresses -- hoisted out of the pass loop they cost 40 registers and, at 16 waves, scratch)
    if constexpr (GROUPED) asm volatile("" : "+v"(wrow), "+v"(wsrow), "+v"(kq32));
    // rows past the end (M, or the group's) alias the pass's first row: they only reach outputs that are never stored
    size_t arow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int row = m0 + mt * 16 + (lane & 15);
      arow[mt] = (size_t)(row < row_end ? row : m0);
    }
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    Stage cur[kChunk], nxt[kChunk];
    issue(cur, ks0);
    for (int step = ks0; step < ks1; step += kChunk) {
      const bool more = step + kChunk < ks1;  // wave-uniform
      if (more) issue(nxt, step + kChunk);
#pragma unroll
      for (int d = 0; d < kChunk; ++d) {
        if (step + d < ks1) {
          const int k0 = (step + d) * 128 + kq32;
          // (16 | K: a block lies inside K or outside; outside, both operands are zero)
          const bool v0 = k0 < p.K, v1 = k0 + 16 < p.K;
          u32x4 w[4];
          decode_blocks(cur[d].q, cur[d].s, has_pw, pw, v0, v1, w);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            u32x4 a[4];
            if constexpr (KIND == kKindWo) {
              const u32x4 z = {0u, 0u, 0u, 0u};
              const uint16_t* xp = p.x + arow[mt] * p.K + (v0 ? k0 : 0);
              const uint16_t* xq = p.x + arow[mt] * p.K + (v1 ? k0 + 16 : 0);
              a[0] = *reinterpret_cast<const u32x4*>(xp);
              a[1] = *reinterpret_cast<const u32x4*>(xp + 8);
              a[2] = *reinterpret_cast<const u32x4*>(xq);
              a[3] = *reinterpret_cast<const u32x4*>(xq + 8);
              if (!v0) a[0] = a[1] = z;
              if (!v1) a[2] = a[3] = z;
            } else {
              u32x4 aq;
              uint32_t as;
              load_blocks<false>(p.a + arow[mt] * (p.K >> 1), p.a_scale + arow[mt] * kb, k0, p.K, k32, aq, as);
              decode_blocks(aq, as, false, 1.f, v0, v1, a);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[mt] = mfma_bf16(a[i], w[i], acc[mt]);
          }
        }
      }
      if (more) {
#pragma unroll
        for (int d = 0; d < kChunk; ++d) cur[d] = nxt[d];
      }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) red[wave][mt][lane] = acc[mt];
    lds_barrier();
    // wave w stores m-tiles w, w + WAVES, ...: the partial tiles are added in wave order
    const bool has_bias = p.bias != nullptr;
    const float bias = (has_bias && n < p.N) ? bf16_lo_to_f32(p.bias[n]) : 0.f;
    bool has_P = false;
    const float P = KIND == kKindDyn ? nvfp4_P(p.pa, p.pb, has_P) : 1.f;
    for (int mt = wave; mt < MT; mt += WAVES) {
      f32x4 c = red[0][mt][lane];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) c += red[w][mt][lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + mt * 16 + 4 * kq + r;
        if (row < row_end && n < p.N) {
          const float v = KIND == kKindWo  ? nvfp4_wo_out(c[r], has_bias, bias)
                          : p.scaled_mm    ? nvfp4_scaled_mm_out(c[r], P)
                                           : nvfp4_mm_out(c[r], has_P, P, has_bias, bias);
          p.out[(size_t)row * p.N + n] = f32_to_bf16_bits(v);
        }
      }
    }
    if constexpr (!GROUPED) break;
    if (m0 + 16 * MT >= row_end) break;  // workgroup-uniform
    lds_barrier();                       // the next pass parks into the same buffer
  }
}

// ---- LDS-tiled form -------------------------------------------------------------------------------------------------------------
// A stage holds 64 rows x 64 k of each operand as bf16, rows 144 bytes apart (128 + 16: the ds_read_b128 of 16 rows x 4 pieces spread over
// the banks).  Thread t stages one block of 16 k (row t >> 2, k at 16 (t & 3)) of each operand: 8 bytes of codes and a scale byte decoded
// to two 16-byte pieces, or (the weight-only activation) two 16-byte pieces of bf16.
constexpr int kTileRow = 144;
constexpr int kTileOp = 64 * kTileRow;

// ONE body, two instantiations per KIND:
//   GROUPED false, "nvfp4_tile_kernel": the dense linear; the tile row is blockIdx.y.
//   GROUPED true, "nvfp4_grouped_tile_kernel": grid y is the host's upper bound ceil(M_total / 64) + E on the 64-row tiles of all groups (a
//     group adds at most one partial tile); a workgroup finds its (group, tile) by walking offs and leaves when it has none; p then becomes
//     the group's row window [row_begin, row_end) against its expert, expressed by offset base pointers, so rows outside the window are
//     staged as zeros and never stored.
template <int KIND, bool GROUPED>
__global__ __launch_bounds__(256) void nvfp4_tile_kernel(Nvfp4Args p) {
  unsigned tile_y = blockIdx.y;
  if constexpr (GROUPED) {
    int t = blockIdx.y, e = 0, row_begin = 0, row_end = 0;
    for (; e < p.E; ++e) {
      group_bounds(p.offs, e, p.M, row_begin, row_end);
      const int tiles = row_end > row_begin ? (row_end - row_begin + 63) >> 6 : 0;
      if (t < tiles) break;
      t -= tiles;
    }
    if (e == p.E) return;
    const int kb = p.K >> 4;
    if constexpr (KIND == kKindWo) {
      p.x += (size_t)row_begin * p.K;
    } else {
      p.a += (size_t)row_begin * (p.K >> 1);
      p.a_scale += (size_t)row_begin * kb;
    }
    // the expert's base in 64 bits: the whole b may pass 2^31 elements
    p.b += (size_t)e * p.N * (p.K >> 1);
    p.b_scale += (size_t)e * p.N * kb;
    if (p.pa != nullptr) p.pa += e;
    if (p.pb != nullptr) p.pb += e;
    p.out += (size_t)row_begin * p.N;
    p.M = row_end - row_begin;
    tile_y = t;
  }
  __shared__ __attribute__((aligned(16))) char smem[2 * kTileOp];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
  const int m0 = tile_y * 64, n0 = blockIdx.x * 64;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int sr = tid >> 2, sp = tid & 3;  // staging row and block
  const int kb = p.K >> 4;
  const bool arow_ok = m0 + sr < p.M, brow_ok = n0 + sr < p.N;
  const size_t ar = arow_ok ? m0 + sr : 0, br = brow_ok ? n0 + sr : 0;
  const bool has_pw = KIND == kKindWo && p.pb != nullptr;
  const float pw = has_pw ? *p.pb : 1.f;
  const int ksteps = (p.K + 63) >> 6;
  const u32x4 z = {0u, 0u, 0u, 0u};
  u32x4 ga0 = z, ga1 = z;
  u32x2 gaq = {0u, 0u}, gb = {0u, 0u};
  uint32_t gas = 0u, gbs = 0u;
  bool gkv = false;
  auto fetch = [&](int step) {
    const int k0 = step * 64 + 16 * sp;
    gkv = k0 < p.K;  // (16 | K)
    if constexpr (KIND == kKindWo) {
      ga0 = (gkv && arow_ok) ? *reinterpret_cast<const u32x4*>(p.x + ar * p.K + k0) : z;
      ga1 = (gkv && arow_ok) ? *reinterpret_cast<const u32x4*>(p.x + ar * p.K + k0 + 8) : z;
    } else {
      gaq = (gkv && arow_ok) ? *reinterpret_cast<const u32x2*>(p.a + ar * (p.K >> 1) + (k0 >> 1)) : u32x2{0u, 0u};
      gas = (gkv && arow_ok) ? (uint32_t)p.a_scale[ar * kb + (k0 >> 4)] : 0u;
    }
    gb = (gkv && brow_ok) ? *reinterpret_cast<const u32x2*>(p.b + br * (p.K >> 1) + (k0 >> 1)) : u32x2{0u, 0u};
    gbs = (gkv && brow_ok) ? (uint32_t)p.b_scale[br * kb + (k0 >> 4)] : 0u;
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  char* sa = smem + sr * kTileRow + sp * 32;
  char* sb = smem + kTileOp + sr * kTileRow + sp * 32;
  fetch(0);
  for (int step = 0; step < ksteps; ++step) {
    // rows past the matrix and blocks past K are zero (not 0 x scale: a scale byte may be NaN)
    u32x4 w0 = z, w1 = z, a0 = ga0, a1 = ga1;
    if (gkv && brow_ok) nvfp4_block16(gb, nvfp4_scale32(gbs, has_pw, pw), w0, w1);
    if constexpr (KIND == kKindDyn) {
      a0 = a1 = z;
      if (gkv && arow_ok) nvfp4_block16(gaq, nvfp4_scale32(gas, false, 1.f), a0, a1);
    }
    __syncthreads();  // every wave is done with the previous stage
    *reinterpret_cast<u32x4*>(sa) = a0;
    *reinterpret_cast<u32x4*>(sa + 16) = a1;
    *reinterpret_cast<u32x4*>(sb) = w0;
    *reinterpret_cast<u32x4*>(sb + 16) = w1;
    __syncthreads();
    if (step + 1 < ksteps) fetch(step + 1);  // in flight under the MFMAs
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      u32x4 bf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        bf[j] = *reinterpret_cast<const u32x4*>(smem + kTileOp + (wn + 16 * j + (lane & 15)) * kTileRow + (4 * kk + kq) * 16);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const u32x4 af = *reinterpret_cast<const u32x4*>(smem + (wm + 16 * i + (lane & 15)) * kTileRow + (4 * kk + kq) * 16);
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma_bf16(af, bf[j], acc[i][j]);
      }
    }
  }
  const bool has_bias = p.bias != nullptr;
  bool has_P = false;
  const float P = KIND == kKindDyn ? nvfp4_P(p.pa, p.pb, has_P) : 1.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + 16 * j + (lane & 15);
    if (n >= p.N) continue;
    const float bias = has_bias ? bf16_lo_to_f32(p.bias[n]) : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + 16 * i + 4 * kq + r;
        if (row < p.M) {
          const float c = acc[i][j][r];
          const float v = KIND == kKindWo  ? nvfp4_wo_out(c, has_bias, bias)
                          : p.scaled_mm    ? nvfp4_scaled_mm_out(c, P)
                                           : nvfp4_mm_out(c, has_P, P, has_bias, bias);
          p.out[(size_t)row * p.N + n] = f32_to_bf16_bits(v);
        }
      }
  }
}

// ---- the cast: one lane per 16-block ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nvfp4_quant_kernel(const uint16_t* __restrict__ x, const float* __restrict__ per_tensor_scale,
                                                          uint8_t* __restrict__ q, uint8_t* __restrict__ s, int64_t blocks) {
  const int64_t blk = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (blk >= blocks) return;
  const bool has_p = per_tensor_scale != nullptr;
  const float p = has_p ? *per_tensor_scale : 1.f;
  const u32x4* px = reinterpret_cast<const u32x4*>(x + blk * 16);
  const u32x4 v[2] = {px[0], px[1]};
  uint32_t s8;
  *reinterpret_cast<u32x2*>(q + blk * 8) = nvfp4_cast16(v, has_p, p, s8);
  s[blk] = (uint8_t)s8;
}

// ---- per-tensor amax -> scale: clear, a vector atomic max over the non-negative bit patterns (a NaN's pattern is above infinity's, so it
// wins as in torch.max), then amax / 2688 in place.  Three launches on the stream, no host read. ---------------------------------------
__global__ void nvfp4_amax_clear_kernel(uint32_t* out) {
  if (threadIdx.x == 0) *out = 0u;
}

__global__ __launch_bounds__(256) void nvfp4_amax_kernel(const uint16_t* __restrict__ x, int64_t pieces, uint32_t* out) {
  const u32x4* px = reinterpret_cast<const u32x4*>(x);
  float m = 0.f;
  bool has_nan = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pieces; i += (int64_t)gridDim.x * 256) m = fmaxf(m, amax8(px[i], has_nan));
  m = wave_max(m);
  const bool any_nan = __ballot(has_nan) != 0ull;
  if ((threadIdx.x & 63) == 0) atomicMax(out, any_nan ? 0x7FC00000u : f32_to_bits(m));
}

__global__ void nvfp4_amax_scale_kernel(uint32_t* out) {
  if (threadIdx.x == 0) *reinterpret_cast<float*>(out) = bits_to_f32(*out) / 2688.0f;
}

// ---- the grouped cast: row r under its group's p[e].  The group is the first e with offs[e] > r (a binary search: offs is cumulative);
// rows past offs[E-1] are not written.  Without p only that end is needed. --------------------------------------------------------------
__global__ __launch_bounds__(256) void nvfp4_quant_grouped_kernel(const uint16_t* __restrict__ x, const float* __restrict__ p,
                                                                  const int32_t* __restrict__ offs, uint8_t* __restrict__ q,
                                                                  uint8_t* __restrict__ s, int64_t blocks, int kb, int E) {
  const int64_t blk = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (blk >= blocks) return;
  const int row = (int)(blk / kb);
  const bool has_p = p != nullptr;
  float ps = 1.f;
  if (has_p) {
    int lo = 0, hi = E;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (offs[mid] > row) hi = mid; else lo = mid + 1;
    }
    if (lo == E) return;
    ps = p[lo];
  } else if (row >= offs[E - 1]) {
    return;
  }
  const u32x4* px = reinterpret_cast<const u32x4*>(x + blk * 16);
  const u32x4 v[2] = {px[0], px[1]};
  uint32_t s8;
  *reinterpret_cast<u32x2*>(q + blk * 8) = nvfp4_cast16(v, has_p, ps, s8);
  s[blk] = (uint8_t)s8;
}

// ---- per-group amax -> scale: as the per-tensor one, out[e] over group e's rows; grid (parts, E).  An empty group stays 0. -------------
__global__ void nvfp4_group_amax_clear_kernel(uint32_t* out, int E) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < E) out[e] = 0u;
}

__global__ __launch_bounds__(256) void nvfp4_group_amax_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ offs, int M_total,
                                                               int K, uint32_t* out) {
  int row_begin, row_end;
  group_bounds(offs, blockIdx.y, M_total, row_begin, row_end);
  if (row_end <= row_begin) return;
  const u32x4* px = reinterpret_cast<const u32x4*>(x + (size_t)row_begin * K);
  const int64_t pieces = (int64_t)(row_end - row_begin) * (K >> 3);
  float m = 0.f;
  bool has_nan = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pieces; i += (int64_t)gridDim.x * 256) m = fmaxf(m, amax8(px[i], has_nan));
  m = wave_max(m);
  const bool any_nan = __ballot(has_nan) != 0ull;
  // (out[e] was cleared to 0: a wave that met nothing above 0 has nothing to add, and E addresses serialize what does arrive)
  if ((threadIdx.x & 63) == 0 && (any_nan || m > 0.f)) atomicMax(out + blockIdx.y, any_nan ? 0x7FC00000u : f32_to_bits(m));
}

__global__ void nvfp4_group_amax_scale_kernel(uint32_t* out, int E) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < E) reinterpret_cast<float*>(out)[e] = bits_to_f32(out[e]) / 2688.0f;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------
// (4 m-tiles x 16 waves: the meeting buffer would pass the static LDS; the stream-form plan caps 4 m-tiles at 8 waves)
template <int KIND>
int launch_stream(const TwoFormRoute& r, const Nvfp4Args& a, hipStream_t st) {
  return launch_stream_form<false>("nvfp4_stream_kernel", "nvfp4_stream_kernel launch", r, a, st, [](auto mt, auto waves) {
    return nvfp4_stream_kernel<KIND, decltype(mt)::value, decltype(waves)::value, false>;
  });
}

template <int KIND>
int launch_tile(const TwoFormRoute& r, const Nvfp4Args& a, hipStream_t st) {
  return launch_tile_form(nvfp4_tile_kernel<KIND, false>, "nvfp4_tile_kernel launch", r, a, st);
}

template <int KIND>
int launch_grouped_stream(const TwoFormRoute& r, const Nvfp4Args& a, hipStream_t st) {
  return launch_stream_form<false>("nvfp4_grouped_stream_kernel", "nvfp4_grouped_stream_kernel (nvfp4_stream_kernel<GROUPED>) launch", r, a, st,
                                   [](auto mt, auto waves) { return nvfp4_stream_kernel<KIND, decltype(mt)::value, decltype(waves)::value, true>; });
}

template <int KIND>
int launch_grouped_tile(const TwoFormRoute& r, const Nvfp4Args& a, hipStream_t st) {
  return launch_tile_form(nvfp4_tile_kernel<KIND, true>, "nvfp4_grouped_tile_kernel (nvfp4_tile_kernel<GROUPED>) launch", r, a, st);
}

// ---- the grouped route ------------------------------------------------------------------------------------------------------------
// (on the mean group size: grouped_two_form_route)
constexpr int kGroupedStreamMaxRows = AO_NVFP4_GROUPED_STREAM_MAX_ROWS;

thread_local int g_grouped_form = 0;  // ao_nvfp4_grouped_mm_set_form: 0 the product route, 1 stream, 2 tile

bool nvfp4_grouped_shape_ok(int kind, int64_t M_total, int64_t N, int64_t K, int64_t E) {
  if (E < 1 || E > 65535) return false;
  return nvfp4_shape_ok(kind, M_total, N, K);  // M_total K and the per-expert N K below 2^31; the expert base is 64-bit
}

// kernel 1: nvfp4_grouped_stream_kernel, grid (ceil(N / 16), E), m-tiles and waves of the stream plan at the mean group size;
// 2: nvfp4_grouped_tile_kernel, grid (ceil(N / 64), ceil(M_total / 64) + E)
TwoFormRoute nvfp4_grouped_route(int kind, int64_t M_total, int64_t N, int64_t K, int64_t E) {
  if (!nvfp4_grouped_shape_ok(kind, M_total, N, K, E)) return TwoFormRoute{};
  return grouped_two_form_route(g_grouped_form, kGroupedStreamMaxRows, M_total, N, K, E, 64);
}

int check_shape(const char* fn, int kind, int64_t M, int64_t N, int64_t K) {
  AO_REQUIRE(nvfp4_shape_ok(kind, M, N, K),
             "%s: bad shape M=%lld N=%lld K=%lld (M >= 0, N >= 1, K a positive multiple of 16 up to 2^31 - 1024, operands < 2^31 elements)", fn,
             (long long)M, (long long)N, (long long)K);
  return AO_OK;
}

template <int KIND>
int run(const char* fn, const Nvfp4Args& args, int64_t M, int64_t N, int64_t K, hipStream_t st) {
  const TwoFormRoute r = nvfp4_route(KIND, M, N, K);
  AO_REQUIRE(r.kernel != 0, "%s: no route for M=%lld N=%lld K=%lld", fn, (long long)M, (long long)N, (long long)K);
  return r.kernel == 1 ? launch_stream<KIND>(r, args, st) : launch_tile<KIND>(r, args, st);
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_nvfp4_amax_scale(const uint16_t* x, float* out, int64_t R, int64_t C, void* stream) {
  AO_REQUIRE(R >= 0 && C > 0 && C % 16 == 0, "%s: bad shape R=%lld C=%lld (C must be a positive multiple of 16)", __func__, (long long)R,
             (long long)C);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(out, 4), "%s: out must be 4-byte aligned", __func__);
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* bits = reinterpret_cast<uint32_t*>(out);
  ao::launch(nvfp4_amax_clear_kernel, dim3(1), dim3(64), 0, s, bits);
  if (R > 0) {
    AO_REQUIRE_PTR(x);
    AO_REQUIRE(aligned_to(x, 16), "%s: x must be 16-byte aligned", __func__);
    const int64_t pieces = R * C / 8;
    const int64_t grid = std::min<int64_t>((pieces + 255) / 256, 1024);
    ao::launch(nvfp4_amax_kernel, dim3((unsigned)grid), dim3(256), 0, s, x, pieces, bits);
  }
  ao::launch(nvfp4_amax_scale_kernel, dim3(1), dim3(64), 0, s, bits);
  AO_LAUNCH_CHECK("nvfp4_amax kernels launch");
  return AO_OK;
}

extern "C" int ao_nvfp4_quantize(const uint16_t* x, const float* per_tensor_scale, uint8_t* q, uint8_t* scale_e4m3, int64_t R, int64_t C,
                                 void* stream) {
  AO_REQUIRE(R >= 0 && C > 0 && C % 16 == 0, "%s: bad shape R=%lld C=%lld (C must be a positive multiple of 16)", __func__, (long long)R,
             (long long)C);
  if (R == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(scale_e4m3);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(q, 8) && aligned_to(per_tensor_scale, 4),
             "%s: x must be 16-byte, q 8-byte and per_tensor_scale 4-byte aligned", __func__);
  const int64_t blocks = R * (C / 16);
  const int64_t grid = (blocks + 255) / 256;
  AO_REQUIRE(grid < (1ll << 31), "%s: tensor too large for one launch", __func__);
  ao::launch(nvfp4_quant_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), x, per_tensor_scale, q, scale_e4m3, blocks);
  AO_LAUNCH_CHECK("nvfp4_quant_kernel launch");
  return AO_OK;
}

extern "C" int ao_nvfp4_linear_route(int kind, int64_t M, int64_t N, int64_t K, int32_t* out, int cap) {
  return route_export(__func__, nvfp4_route(kind, M, N, K), out, cap);
}

extern "C" const char* ao_nvfp4_linear_kernel_name(int kind, int64_t M, int64_t N, int64_t K) {
  return route_kernel_name(nvfp4_route(kind, M, N, K), "nvfp4_stream_kernel", "nvfp4_tile_kernel");
}

extern "C" int ao_nvfp4_linear_set_form(int form) { return set_forced_form(__func__, form, g_form); }

extern "C" int ao_nvfp4_wo_linear(const uint16_t* x, const uint8_t* wq, const uint8_t* w_scale, const float* w_per_tensor_scale,
                                  const uint16_t* bias, uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream) {
  if (int rc = check_shape(__func__, kKindWo, M, N, K)) return rc;
  AO_REQUIRE_PTR(wq);
  AO_REQUIRE_PTR(w_scale);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(out);
  // (K a multiple of 32: rows of codes are read 16 bytes and scales two at a time; otherwise 8 bytes and one)
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(wq, K % 32 ? 8 : 16) && aligned_to(w_scale, K % 32 ? 1 : 2),
             "%s: x must be 16-byte aligned, the codes 16-byte and the block scales 2-byte (K %% 32 != 0: 8-byte and 1-byte)", __func__);
  AO_REQUIRE(aligned_to(w_per_tensor_scale, 4) && aligned_to(bias, 2) && aligned_to(out, 2),
             "%s: the per-tensor scale must be 4-byte, bias and out 2-byte aligned", __func__);
  const Nvfp4Args args{x, nullptr, nullptr, wq, w_scale, nullptr, w_per_tensor_scale, bias, out, (int)M, (int)N, (int)K};
  return run<kKindWo>(__func__, args, M, N, K, static_cast<hipStream_t>(stream));
}

extern "C" int ao_nvfp4_linear(const uint8_t* a, const uint8_t* a_scale, const float* a_per_tensor_scale, const uint8_t* b, const uint8_t* b_scale,
                               const float* b_per_tensor_scale, const uint16_t* bias, uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream) {
  if (int rc = check_shape(__func__, kKindDyn, M, N, K)) return rc;
  AO_REQUIRE_PTR(b);
  AO_REQUIRE_PTR(b_scale);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(a);
  AO_REQUIRE_PTR(a_scale);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(a, K % 32 ? 8 : 16) && aligned_to(b, K % 32 ? 8 : 16) && aligned_to(a_scale, K % 32 ? 1 : 2) && aligned_to(b_scale, K % 32 ? 1 : 2),
             "%s: the codes must be 16-byte and the block scales 2-byte aligned (K %% 32 != 0: 8-byte and 1-byte)", __func__);
  AO_REQUIRE(aligned_to(a_per_tensor_scale, 4) && aligned_to(b_per_tensor_scale, 4) && aligned_to(bias, 2) && aligned_to(out, 2),
             "%s: the per-tensor scales must be 4-byte, bias and out 2-byte aligned", __func__);
  const Nvfp4Args args{nullptr, a, a_scale, b, b_scale, a_per_tensor_scale, b_per_tensor_scale, bias, out, (int)M, (int)N, (int)K};
  return run<kKindDyn>(__func__, args, M, N, K, static_cast<hipStream_t>(stream));
}

// The training GEMMs (prototype/moe_training/nvfp4_training/nvfp4_linear.py:213-223, :278-306: torch.nn.functional.scaled_mm on e2m1
// codes with BlockWise1x16 + TensorWise scales): the codes x codes route and bodies above under the scaled_mm epilogue.
extern "C" int ao_nvfp4_scaled_mm(const uint8_t* a, const uint8_t* a_scale, const float* pa, const uint8_t* b, const uint8_t* b_scale, const float* pb,
                                  uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream) {
  if (int rc = check_shape(__func__, kKindDyn, M, N, K)) return rc;
  AO_REQUIRE_PTR(b);
  AO_REQUIRE_PTR(b_scale);
  AO_REQUIRE_PTR(pa);
  AO_REQUIRE_PTR(pb);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(a);
  AO_REQUIRE_PTR(a_scale);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(a, K % 32 ? 8 : 16) && aligned_to(b, K % 32 ? 8 : 16) && aligned_to(a_scale, K % 32 ? 1 : 2) && aligned_to(b_scale, K % 32 ? 1 : 2),
             "%s: the codes must be 16-byte and the block scales 2-byte aligned (K %% 32 != 0: 8-byte and 1-byte)", __func__);
  AO_REQUIRE(aligned_to(pa, 4) && aligned_to(pb, 4) && aligned_to(out, 2), "%s: the per-tensor scales must be 4-byte, out 2-byte aligned", __func__);
  const Nvfp4Args args{nullptr, a, a_scale, b, b_scale, pa, pb, nullptr, out, (int)M, (int)N, (int)K, nullptr, 0, 1};
  return run<kKindDyn>(__func__, args, M, N, K, static_cast<hipStream_t>(stream));
}

// ---- grouped (MoE experts) ----------------------------------------------------------------------------------------------------------
extern "C" int ao_nvfp4_grouped_mm_route(int kind, int64_t M_total, int64_t N, int64_t K, int64_t E, int32_t* out, int cap) {
  return route_export(__func__, nvfp4_grouped_route(kind, M_total, N, K, E), out, cap);
}

extern "C" const char* ao_nvfp4_grouped_mm_kernel_name(int kind, int64_t M_total, int64_t N, int64_t K, int64_t E) {
  return route_kernel_name(nvfp4_grouped_route(kind, M_total, N, K, E), "nvfp4_grouped_stream_kernel", "nvfp4_grouped_tile_kernel");
}

extern "C" int ao_nvfp4_grouped_mm_set_form(int form) { return set_forced_form(__func__, form, g_grouped_form); }

extern "C" int ao_nvfp4_grouped_mm(int kind, const uint16_t* x, const uint8_t* a, const uint8_t* a_scale, const uint8_t* b, const uint8_t* b_scale,
                                   const float* pa, const float* pb, const int32_t* offs, uint16_t* out, int64_t M_total, int64_t N, int64_t K,
                                   int64_t E, void* stream) {
  AO_REQUIRE(nvfp4_grouped_shape_ok(kind, M_total, N, K, E),
             "%s: bad kind or shape kind=%d M_total=%lld N=%lld K=%lld E=%lld (kind 0 or 1, M_total >= 0, N >= 1, K a positive multiple of 16, "
             "1 <= E <= 65535, M_total K and the per-expert N K < 2^31)",
             __func__, kind, (long long)M_total, (long long)N, (long long)K, (long long)E);
  AO_REQUIRE_PTR(b);
  AO_REQUIRE_PTR(b_scale);
  AO_REQUIRE_PTR(offs);
  AO_REQUIRE(kind == kKindDyn || pa == nullptr, "%s: the weight-only kind takes no activation scale pa", __func__);
  if (M_total == 0) return AO_OK;
  if (kind == kKindWo) {
    AO_REQUIRE_PTR(x);
    AO_REQUIRE(aligned_to(x, 16), "%s: x must be 16-byte aligned", __func__);
  } else {
    AO_REQUIRE_PTR(a);
    AO_REQUIRE_PTR(a_scale);
    AO_REQUIRE(aligned_to(a, K % 32 ? 8 : 16) && aligned_to(a_scale, K % 32 ? 1 : 2),
               "%s: the activation codes must be 16-byte and their block scales 2-byte aligned (K %% 32 != 0: 8-byte and 1-byte)", __func__);
  }
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(b, K % 32 ? 8 : 16) && aligned_to(b_scale, K % 32 ? 1 : 2),
             "%s: the weight codes must be 16-byte and their block scales 2-byte aligned (K %% 32 != 0: 8-byte and 1-byte)", __func__);
  AO_REQUIRE(aligned_to(pa, 4) && aligned_to(pb, 4) && aligned_to(offs, 4) && aligned_to(out, 2),
             "%s: the per-expert scales and offs must be 4-byte, out 2-byte aligned", __func__);
  const TwoFormRoute r = nvfp4_grouped_route(kind, M_total, N, K, E);
  AO_REQUIRE(r.kernel != 0, "%s: no route for M_total=%lld N=%lld K=%lld E=%lld (more than 65535 grid rows)", __func__, (long long)M_total,
             (long long)N, (long long)K, (long long)E);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (kind == kKindWo) {
    const Nvfp4Args args{x, nullptr, nullptr, b, b_scale, nullptr, pb, nullptr, out, (int)M_total, (int)N, (int)K, offs, (int)E};
    return r.kernel == 1 ? launch_grouped_stream<kKindWo>(r, args, st) : launch_grouped_tile<kKindWo>(r, args, st);
  }
  const Nvfp4Args args{nullptr, a, a_scale, b, b_scale, pa, pb, nullptr, out, (int)M_total, (int)N, (int)K, offs, (int)E};
  return r.kernel == 1 ? launch_grouped_stream<kKindDyn>(r, args, st) : launch_grouped_tile<kKindDyn>(r, args, st);
}

namespace {
int check_grouped_rows(const char* fn, int64_t M_total, int64_t K, int64_t E) {
  AO_REQUIRE(M_total >= 0 && K > 0 && K % 16 == 0 && E >= 1 && E <= 65535 && M_total < (1ll << 31) && K < (1ll << 31) && M_total * K < (1ll << 40),
             "%s: bad shape M_total=%lld K=%lld E=%lld (M_total >= 0, K a positive multiple of 16, 1 <= E <= 65535)", fn, (long long)M_total,
             (long long)K, (long long)E);
  return AO_OK;
}
}  // namespace

extern "C" int ao_nvfp4_group_amax_scale(const uint16_t* x, const int32_t* offs, float* out, int64_t M_total, int64_t K, int64_t E, void* stream) {
  if (int rc = check_grouped_rows(__func__, M_total, K, E)) return rc;
  AO_REQUIRE_PTR(offs);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(out, 4) && aligned_to(offs, 4), "%s: out and offs must be 4-byte aligned", __func__);
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* bits = reinterpret_cast<uint32_t*>(out);
  const unsigned eg = (unsigned)((E + 255) / 256);
  ao::launch(nvfp4_group_amax_clear_kernel, dim3(eg), dim3(256), 0, s, bits, (int)E);
  if (M_total > 0) {
    AO_REQUIRE_PTR(x);
    AO_REQUIRE(aligned_to(x, 16), "%s: x must be 16-byte aligned", __func__);
    // parts per group: one pass of 256 lanes over a group of the mean size (a larger group takes more passes of its grid-stride loop)
    const int64_t pieces = M_total * K / 8;
    const int64_t parts = std::max<int64_t>(1, std::min<int64_t>({(pieces / E + 255) / 256, 1024, (16384 + E - 1) / E}));
    ao::launch(nvfp4_group_amax_kernel, dim3((unsigned)parts, (unsigned)E), dim3(256), 0, s, x, offs, (int)M_total, (int)K, bits);
  }
  ao::launch(nvfp4_group_amax_scale_kernel, dim3(eg), dim3(256), 0, s, bits, (int)E);
  AO_LAUNCH_CHECK("nvfp4_group_amax kernels launch");
  return AO_OK;
}

extern "C" int ao_nvfp4_quantize_grouped(const uint16_t* x, const float* p, const int32_t* offs, uint8_t* q, uint8_t* scale_e4m3, int64_t M_total,
                                         int64_t K, int64_t E, void* stream) {
  if (int rc = check_grouped_rows(__func__, M_total, K, E)) return rc;
  AO_REQUIRE_PTR(offs);
  if (M_total == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(scale_e4m3);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(q, 8) && aligned_to(p, 4) && aligned_to(offs, 4),
             "%s: x must be 16-byte, q 8-byte, p and offs 4-byte aligned", __func__);
  const int64_t blocks = M_total * (K / 16);
  const int64_t grid = (blocks + 255) / 256;
  AO_REQUIRE(grid < (1ll << 31), "%s: tensor too large for one launch", __func__);
  ao::launch(nvfp4_quant_grouped_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), x, p, offs, q, scale_e4m3, blocks,
             (int)(K / 16), (int)E);
  AO_LAUNCH_CHECK("nvfp4_quant_grouped_kernel launch");
  return AO_OK;
}
