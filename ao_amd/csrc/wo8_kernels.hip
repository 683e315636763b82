// int8 / float8 (e4m3fn) WEIGHT-ONLY linears for gfx950: bf16 activation x 8-bit weight, the reference's weight-only arithmetic.
//
// Replaces the weight-only branch of Int8Tensor's F.linear (quantize_/workflows/int8/int8_tensor.py:346-359: torch.mm(x, qdata.t().to(bf16))
// * scale.to(bf16) + bias, per-row / per-tensor) and of Float8Tensor's (quantize_/workflows/float8/float8_tensor.py:460-469:
// torch.matmul(x, weight.dequantize()) + bias, with dequantize :255-275).  The arithmetic (quant_math.h: wo8_weight16, wo8_out):
//   int8: t = bf16(sum_k x q);  u = bf16(f32(t) f32(bf16(s[n])));  y = bf16(f32(u) + bias[n])
//   e4m3: w = bf16(f32(q) s[n]);  t = bf16(sum_k x w);  y = bf16(f32(t) + bias[n])
// fp32 accumulation in v_mfma_f32_16x16x32_bf16.  The weight becomes bf16 in registers: exactly for int8, by the reference's own
// per-element rounding for e4m3.  The MFMA sums over k in whatever order its lanes hold it, so lane l takes 16 consecutive k of row
// l & 15 -- one 16-byte weight load, two 16-byte activation loads -- and feeds two MFMAs (k 0..7 and 8..15 of its piece).
//
// Two forms, one route (wo8_route: this family's shape check, seams and forced form over the plans of two_form_route.h)
// read by the launch and by ao_wo8_linear_route:
//   wo8_stream_kernel: the weight is streamed once, 1 byte per weight.  A workgroup owns 16 columns and splits K over its waves in runs of
//     128-k steps; a step's two loads of a lane (pieces kq and 4 + kq) complete 128-byte lines, nontemporal; a wave requests a chunk of
//     four steps ahead of the chunk it multiplies.  The activation is read from global memory inside the multiply, behind those requests
//     in the same in-order vmcnt queue, so a chunk's first multiply waits for everything requested so far: the requests of a wave overlap
//     one another and the other waves' multiplies, not its own (what dec8_kernel avoids by holding the activation in
//     LDS).  The partial tiles meet in LDS in wave order behind a barrier that waits for LDS only.  Up to 64 rows per workgroup (MT
//     m-tiles of 16); more rows add grid rows (forced form only).
//   wo8_tile_kernel: 64 x 64 output tiles, four waves of 32 x 32, both operands staged in LDS as bf16 -- the weight converted ONCE, by
//     the thread that stages it -- with the next k step's global loads in flight under the MFMAs.  A first cut: correct for every M,
//     ragged N and K; not tuned.
#include "common.h"
#include "quant_math.h"
#include "two_form_route.h"

#include <algorithm>

namespace ao {
namespace {

constexpr int kFmtInt8 = AO_WO8_FMT_INT8;
constexpr int kFmtE4M3 = AO_WO8_FMT_E4M3;

// ---- the route ------------------------------------------------------------------------------------------------------------------
// Chosen on the Llama-3-8B five shapes (profiles/wo8_linear.jsonl: its "fit" lines, tools/bench_wo8_linear.py --sweep, both forms forced at M = 1 .. 256,
// weights from HBM; --fit sums the five shapes over every swept M per candidate seam): the streaming form up to these rows, the LDS-tiled
// form beyond.  The sum is flat between 64 and 96 rows -- int8 3393 us at 64, 3363 at 65, 3391 at 96; e4m3 3420 / 3382 / 3403 -- and
// rises on both sides (3498 at 48, 3472 at 128).  The fit's minimum is 65; inside the flat region the constants take 64, the last row count the stream form serves with ONE grid row, the weight read once.
// (At 64 rows the five shapes take 256 us streamed, 361 us tiled (int8); at 128 rows 440 vs 359.  Per shape the seams differ: gate / up
// are level from 33 rows, down stays ahead streamed to 128.)
constexpr int kStreamMaxRowsInt8 = 64;
constexpr int kStreamMaxRowsE4M3 = 64;

thread_local int g_form = 0;  // ao_wo8_linear_set_form: 0 the product route, 1 stream, 2 tile

bool wo8_shape_ok(int fmt, int64_t M, int64_t N, int64_t K) {
  if (fmt != kFmtInt8 && fmt != kFmtE4M3) return false;
  if (M < 0 || N < 1 || K < 16 || K % 16 != 0) return false;
  // K + 1024 below 2^31: the kernels walk k in 32-bit steps of up to 128 past the last one of a chunk
  if (M >= (1ll << 31) || N >= (1ll << 31) || K > (1ll << 31) - 1024) return false;
  return M * K < (1ll << 31) && N * K < (1ll << 31) && M * N < (1ll << 40);
}

// kernel 1: wo8_stream_kernel, 2: wo8_tile_kernel (64 x 64 tiles)
TwoFormRoute wo8_route(int fmt, int64_t M, int64_t N, int64_t K) {
  if (!wo8_shape_ok(fmt, M, N, K)) return TwoFormRoute{};
  const int seam = fmt == kFmtInt8 ? kStreamMaxRowsInt8 : kStreamMaxRowsE4M3;
  TwoFormRoute r = two_form_route(g_form != 0 ? g_form : (M <= seam ? 1 : 2), M, N, K, 64);
  r.grid_y = std::max(r.grid_y, 1);  // (this family's tiled form reports one grid row at M = 0 -- a forced form only; never launched)
  return r;
}

struct Wo8Args {
  const uint16_t* x;     // bf16 [M][K]
  const uint8_t* w;      // codes [N][K]
  const float* scale;    // fp32 [N] or [1]
  const uint16_t* bias;  // bf16 [N] or null
  uint16_t* out;         // bf16 [M][N]
  int M, N, K;
  int per_tensor;        // one scale for every row
};

__device__ __forceinline__ f32x4 mfma_bf16(const u32x4& a, const u32x4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- streaming form -------------------------------------------------------------------------------------------------------------
constexpr int kChunk = 4;  // 128-k steps a wave requests at once

template <int FMT, int MT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void wo8_stream_kernel(Wo8Args p) {
  __shared__ f32x4 red[WAVES][MT][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kq = lane >> 4;
  const int n = blockIdx.x * 16 + (lane & 15);
  const int m0 = blockIdx.y * 16 * MT;
  const int ksteps = (p.K + 127) >> 7;
  const int ks0 = (ksteps * wave) / WAVES, ks1 = (ksteps * (wave + 1)) / WAVES;
  // columns past N read the last row (never stored); pieces past K read the row's first piece and are zeroed
  const uint8_t* wrow = p.w + (size_t)min(n, p.N - 1) * p.K;
  const float s = FMT == kFmtE4M3 ? p.scale[p.per_tensor ? 0 : min(n, p.N - 1)] : 0.f;
  // rows past M alias the tile's first row: they only reach outputs that are never stored
  const uint16_t* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = m0 + mt * 16 + (lane & 15);
    xrow[mt] = p.x + (size_t)(row < p.M ? row : m0) * p.K;
  }
  struct Stage {
    u32x4 b0, b1;
  };
  auto issue = [&](Stage (&st)[kChunk], int step) {
#pragma unroll
    for (int d = 0; d < kChunk; ++d) {
      const int k0 = (step + d) * 128 + 16 * kq;
      st[d].b0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow + (k0 < p.K ? k0 : 0)));
      st[d].b1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow + (k0 + 64 < p.K ? k0 + 64 : 0)));
    }
    __builtin_amdgcn_sched_barrier(0);  // every request of the chunk is out before anything waits
  };
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
        const int k0 = (step + d) * 128 + 16 * kq;
        // (16 | K: a piece lies inside K or outside; outside, both operands are zero)
        const bool v0 = k0 < p.K, v1 = k0 + 64 < p.K;
        u32x4 w00 = {0u, 0u, 0u, 0u}, w01 = w00, w10 = w00, w11 = w00;
        if (v0) wo8_weight16<FMT == kFmtInt8>(cur[d].b0, s, w00, w01);
        if (v1) wo8_weight16<FMT == kFmtInt8>(cur[d].b1, s, w10, w11);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const u32x4 z = {0u, 0u, 0u, 0u};
          const uint16_t* xp = xrow[mt] + (v0 ? k0 : 0);
          const uint16_t* xq = xrow[mt] + (v1 ? k0 + 64 : 0);
          u32x4 a00 = *reinterpret_cast<const u32x4*>(xp), a01 = *reinterpret_cast<const u32x4*>(xp + 8);
          u32x4 a10 = *reinterpret_cast<const u32x4*>(xq), a11 = *reinterpret_cast<const u32x4*>(xq + 8);
          if (!v0) a00 = a01 = z;
          if (!v1) a10 = a11 = z;
          acc[mt] = mfma_bf16(a00, w00, acc[mt]);
          acc[mt] = mfma_bf16(a01, w01, acc[mt]);
          acc[mt] = mfma_bf16(a10, w10, acc[mt]);
          acc[mt] = mfma_bf16(a11, w11, acc[mt]);
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
  const float sc = (FMT == kFmtInt8 && n < p.N) ? p.scale[p.per_tensor ? 0 : n] : 0.f;
  for (int mt = wave; mt < MT; mt += WAVES) {
    f32x4 c = red[0][mt][lane];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) c += red[w][mt][lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + mt * 16 + 4 * kq + r;
      if (row < p.M && n < p.N) p.out[(size_t)row * p.N + n] = f32_to_bf16_bits(wo8_out<FMT == kFmtInt8>(c[r], sc, has_bias, bias));
    }
  }
}

// ---- LDS-tiled form -------------------------------------------------------------------------------------------------------------
// A stage holds 64 rows x 64 k of each operand as bf16, rows 144 bytes apart (128 + 16: the ds_read_b128 of 16 rows x 4 pieces spread over
// the banks).  Thread t stages two 16-byte pieces of the activation (row t >> 2, pieces 2 (t & 3), + 1) and one 16-byte piece of codes
// (row t >> 2, 16 k at 16 (t & 3)), which it converts to two bf16 pieces.
constexpr int kTileRow = 144;
constexpr int kTileOp = 64 * kTileRow;

template <int FMT>
__global__ __launch_bounds__(256) void wo8_tile_kernel(Wo8Args p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kTileOp];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int sr = tid >> 2, sp = tid & 3;  // staging row and 16-k piece
  const bool arow_ok = m0 + sr < p.M, brow_ok = n0 + sr < p.N;
  const uint16_t* xa = p.x + (size_t)(arow_ok ? m0 + sr : 0) * p.K;
  const uint8_t* wb = p.w + (size_t)(brow_ok ? n0 + sr : 0) * p.K;
  const float s = FMT == kFmtE4M3 ? p.scale[p.per_tensor || !brow_ok ? 0 : n0 + sr] : 0.f;
  const int ksteps = (p.K + 63) >> 6;
  const u32x4 z = {0u, 0u, 0u, 0u};
  u32x4 ga0, ga1, gb;
  auto fetch = [&](int step) {
    const int k0 = step * 64 + 16 * sp;
    const bool kv = k0 < p.K;  // (16 | K)
    ga0 = (kv && arow_ok) ? *reinterpret_cast<const u32x4*>(xa + k0) : z;
    ga1 = (kv && arow_ok) ? *reinterpret_cast<const u32x4*>(xa + k0 + 8) : z;
    gb = (kv && brow_ok) ? *reinterpret_cast<const u32x4*>(wb + k0) : z;
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
    u32x4 w0, w1;
    wo8_weight16<FMT == kFmtInt8>(gb, s, w0, w1);  // zero codes give zero weights in both formats
    if (FMT == kFmtE4M3 && !brow_ok) w0 = w1 = z;  // (a scale that is not finite would turn them into NaN)
    __syncthreads();  // every wave is done with the previous stage
    *reinterpret_cast<u32x4*>(sa) = ga0;
    *reinterpret_cast<u32x4*>(sa + 16) = ga1;
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
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + 16 * j + (lane & 15);
    if (n >= p.N) continue;
    const float bias = has_bias ? bf16_lo_to_f32(p.bias[n]) : 0.f;
    const float sc = FMT == kFmtInt8 ? p.scale[p.per_tensor ? 0 : n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + 16 * i + 4 * kq + r;
        if (row < p.M) p.out[(size_t)row * p.N + n] = f32_to_bf16_bits(wo8_out<FMT == kFmtInt8>(acc[i][j][r], sc, has_bias, bias));
      }
  }
}

// ---- launches -------------------------------------------------------------------------------------------------------------------
// (4 m-tiles x 16 waves: the meeting buffer would pass the static LDS; the stream-form plan caps 4 m-tiles at 8 waves)
template <int FMT>
int launch_stream(const TwoFormRoute& r, const Wo8Args& a, hipStream_t st) {
  return launch_stream_form<false>("wo8_stream_kernel", "wo8_stream_kernel launch", r, a, st, [](auto mt, auto waves) {
    return wo8_stream_kernel<FMT, decltype(mt)::value, decltype(waves)::value>;
  });
}

template <int FMT>
int launch_tile(const TwoFormRoute& r, const Wo8Args& a, hipStream_t st) {
  return launch_tile_form(wo8_tile_kernel<FMT>, "wo8_tile_kernel launch", r, a, st);
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_wo8_linear_route(int fmt, int64_t M, int64_t N, int64_t K, int32_t* out, int cap) {
  return route_export(__func__, wo8_route(fmt, M, N, K), out, cap);
}

extern "C" int ao_wo8_linear_set_form(int form) { return set_forced_form(__func__, form, g_form); }

extern "C" int ao_wo8_linear(int fmt, const uint16_t* x, const void* wq, const float* w_scale, int64_t scale_count, const uint16_t* bias,
                             uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream) {
  AO_REQUIRE(fmt == kFmtInt8 || fmt == kFmtE4M3, "%s: fmt must be AO_WO8_FMT_INT8 (0) or AO_WO8_FMT_E4M3 (1), got %d", __func__, fmt);
  AO_REQUIRE(wo8_shape_ok(fmt, M, N, K), "%s: bad shape M=%lld N=%lld K=%lld (M >= 0, N >= 1, K a positive multiple of 16 up to 2^31 - 1024, operands < 2^31 elements)",
             __func__, (long long)M, (long long)N, (long long)K);
  AO_REQUIRE(scale_count == N || scale_count == 1, "%s: scale_count must be N (per row) or 1 (per tensor), got %lld", __func__,
             (long long)scale_count);
  AO_REQUIRE_PTR(wq);
  AO_REQUIRE_PTR(w_scale);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(wq, 16), "%s: x and the codes must be 16-byte aligned", __func__);
  AO_REQUIRE(aligned_to(w_scale, 4) && aligned_to(bias, 2) && aligned_to(out, 2), "%s: w_scale must be 4-byte, bias and out 2-byte aligned", __func__);
  const TwoFormRoute r = wo8_route(fmt, M, N, K);
  AO_REQUIRE(r.kernel != 0, "%s: no route for M=%lld N=%lld K=%lld", __func__, (long long)M, (long long)N, (long long)K);
  const Wo8Args args{x, static_cast<const uint8_t*>(wq), w_scale, bias, out, (int)M, (int)N, (int)K, scale_count == 1 ? 1 : 0};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (r.kernel == 1) return fmt == kFmtInt8 ? launch_stream<kFmtInt8>(r, args, st) : launch_stream<kFmtE4M3>(r, args, st);
  return fmt == kFmtInt8 ? launch_tile<kFmtInt8>(r, args, st) : launch_tile<kFmtE4M3>(r, args, st);
}
