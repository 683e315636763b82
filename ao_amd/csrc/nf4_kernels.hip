// NF4 (QLoRA) weights for gfx950: 4-bit codes into a 16-entry table, one int8 scaler per block of B elements, one bf16 quantization
// factor per SB blocks, one bf16 mean.
//
// Replaces, of torchao's NF4Tensor (quantization/quantize_/workflows/nf4/nf4_tensor.py): the cast (from_tensor :649-718, some 25 eager
// ops with a [chunk, 16] broadcast subtract), get_original_weight (:845-871, a dozen more) and LinearNF4's forward at decode row counts
// (:1053-1058: dequantize the whole weight, then F.linear).  The arithmetic contracts are stated once, in quant_math.h ("NF4").
//
//   nf4_absmax_kernel: a[b] = max |x| over block b; B / 8 lanes a block, 16 bytes a lane.
//   nf4_quantize_kernel: ONE launch, two kinds of workgroup: the first `code_grid` write the codes (a lane takes 8 elements of one
//     block: eight divisions, 8 x 16 rounded differences), the rest take one scaler block a wave (m, the factor, the int8 scalers).
//     The mean between the two launches is torch's (the only order-dependent value of the format), read through its pointer.
//   nf4_dequantize_kernel: a flat stream, 8 weights a lane (4 bytes of codes in, 16 bytes out); knows nothing of rows.
//   nf4_stream_kernel: the weight-streaming linear on the plan of two_form_route.h -- a workgroup owns 16 columns and splits K over its
//     waves in runs of 128-k steps; lane (column l & 15, group kq) takes the 32 k at 32 kq of a step: 16 bytes of codes straight from
//     the tensor's quantized_data, HALF a block or less (B >= 32), so one int8 scaler and one factor per lane per step and no shuffles.
//     Codes are looked up in a 16-entry fp32 table in LDS (16 banks: no conflicts, equal codes broadcast), multiplied by the scaler
//     and rounded to bf16 two at a time in front of v_mfma_f32_16x16x32_bf16.  The partial tiles meet in LDS in wave order.
// There is no LDS-tiled form: above the seam the route says "not fused" and the caller runs nf4_dequantize_kernel and a bf16 GEMM.
#include "common.h"
#include "quant_math.h"
#include "two_form_route.h"

#include <algorithm>

namespace ao {
namespace {

// ---- the route ------------------------------------------------------------------------------------------------------------------
// The stream form up to these rows; beyond, dequantize + bf16 GEMM (kernel 0).  Chosen on the Llama-3-8B five shapes
// (profiles/nf4_linear.jsonl: its "fit" line, tools/bench_nf4_linear.py --sweep, the fused form forced and dequantize + F.linear at
// M = 1 .. 256, weights from HBM, three windows a cell, the five shapes summed over every swept M per candidate seam): 3014.5 us at 64,
// 3028.1 at 48, 3058.2 at 65, rising on both sides (3441.9 at 16, 3288.9 at 128; 4165.7 never fused).  At 64 rows the five shapes take
// 245.5 us fused against 259.0 us, at 65 rows 308.2 against 264.5; the windows of a row count spread by 2 - 3 us.  64 is also the last
// row count the stream form serves with ONE grid row.
constexpr int kStreamMaxRows = 64;

thread_local int g_form = 0;  // ao_nf4_linear_set_form: 0 the product route, 1 the stream form at any M

int log2_exact(int64_t v) {
  int l = 0;
  while ((1ll << l) < v) ++l;
  return l;
}

bool nf4_format_ok(int64_t numel, int64_t B, int64_t SB) {
  if (B != 32 && B != 64 && B != 128) return false;
  if (SB < 1 || SB > (1ll << 31) || (SB & (SB - 1)) != 0) return false;
  return numel >= 0 && numel < (1ll << 31) && numel % (B * SB) == 0;
}

// what nf4_stream_kernel takes: blocks inside rows, 32-bit element counts (K + 1024 below 2^31: k walks in 32-bit steps of up to 128
// past the last one of a chunk)
bool nf4_linear_shape_ok(int64_t M, int64_t N, int64_t K, int64_t B, int64_t SB) {
  if (M < 0 || N < 1 || K < 1 || M >= (1ll << 31) || N >= (1ll << 31) || K > (1ll << 31) - 1024) return false;
  if (N * K >= (1ll << 31) || !nf4_format_ok(N * K, B, SB) || K % B != 0) return false;
  return M * K < (1ll << 31) && M * N < (1ll << 40);
}

// kernel 1: nf4_stream_kernel; 0: not fused (dequantize, then multiply) -- above the seam, and for shapes the kernel does not take
TwoFormRoute nf4_route(int64_t M, int64_t N, int64_t K, int64_t B, int64_t SB) {
  if (!nf4_linear_shape_ok(M, N, K, B, SB)) return TwoFormRoute{};
  if (g_form == 0 && M > kStreamMaxRows) return TwoFormRoute{};
  return two_form_route(1, M, N, K, 0);
}

struct Nf4Args {
  const uint16_t* x;     // bf16 [M][K]
  const uint8_t* codes;  // [N][K/2], element 2i in the high nibble
  const int8_t* q;       // [N K / B]
  const uint16_t* qf;    // bf16 [N K / (B SB)]
  const uint16_t* mean;  // bf16, one
  uint16_t* out;         // bf16 [M][N]
  int M, N, K;
  int lb, lsb;  // log2 B, log2 SB
};

__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? bits_to_f32(0x7FC00000u) : fmaxf(a, b); }

__device__ __forceinline__ f32x4 mfma_bf16(const u32x4& a, const u32x4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- the cast -------------------------------------------------------------------------------------------------------------------
// lane t: the 8 elements at 8 t; the 2^lp lanes of a block (lp = log2 B - 3: 4, 8 or 16 lanes, inside one row of 16) meet by shuffles
__global__ __launch_bounds__(256) void nf4_absmax_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ a, int64_t pieces, int lp) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool has_nan = false;
  float m = 0.f;
  if (t < pieces) m = amax8(reinterpret_cast<const u32x4*>(x)[t], has_nan);
  if (has_nan) m = bits_to_f32(0x7FC00000u);
  for (int off = 1; off < (1 << lp); off <<= 1) m = nan_max(m, __shfl_xor(m, off));
  if (t < pieces && (t & ((1 << lp) - 1)) == 0) a[t >> lp] = f32_to_bf16_bits(m);  // (|bf16|: exact)
}

__global__ __launch_bounds__(256) void nf4_quantize_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ a,
                                                           const uint16_t* __restrict__ mean, uint32_t* __restrict__ codes,
                                                           int8_t* __restrict__ q, uint16_t* __restrict__ qf, int64_t pieces,
                                                           int64_t scaler_blocks, int lb, int lsb, unsigned code_grid) {
  if (blockIdx.x < code_grid) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= pieces) return;
    codes[t] = nf4_cast8(reinterpret_cast<const u32x4*>(x)[t], bf16_lo_to_f32(a[t >> (lb - 3)]));
    return;
  }
  // one scaler block a wave
  const int lane = threadIdx.x & 63;
  const int64_t sb = (int64_t)(blockIdx.x - code_grid) * 4 + (threadIdx.x >> 6);
  if (sb >= scaler_blocks) return;
  const float mu = bf16_lo_to_f32(*mean);
  const int64_t b0 = sb << lsb, SB = 1ll << lsb;
  float m = 0.f;
  bool has_nan = false;
  for (int64_t i = lane; i < SB; i += 64) {
    const float c = fabsf(nf4_centred(bf16_lo_to_f32(a[b0 + i]), mu));
    has_nan |= c != c;
    m = fmaxf(m, c);
  }
  m = wave_max(m);
  if (__ballot(has_nan) != 0ull) m = bits_to_f32(0x7FC00000u);
  const float f = nf4_factor(m);
  if (lane == 0) qf[sb] = f32_to_bf16_bits(f);
  for (int64_t i = lane; i < SB; i += 64) q[b0 + i] = (int8_t)nf4_scaler_q(nf4_centred(bf16_lo_to_f32(a[b0 + i]), mu), f);
}

// ---- dequantize: lane t writes the 8 weights at 8 t --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nf4_dequantize_kernel(const uint32_t* __restrict__ codes, const int8_t* __restrict__ q,
                                                             const uint16_t* __restrict__ qf, const uint16_t* __restrict__ mean,
                                                             u32x4* __restrict__ w, int64_t pieces, int lb, int lsb) {
  __shared__ float tab[16];
  if (threadIdx.x < 16) tab[threadIdx.x] = nf4_value(threadIdx.x);
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= pieces) return;
  const int64_t b = t >> (lb - 3);
  const float s = nf4_scaler(q[b], bf16_lo_to_f32(qf[b >> lsb]), bf16_lo_to_f32(*mean));
  w[t] = nf4_decode8(codes[t], s, tab);
}

// ---- the streaming linear ----------------------------------------------------------------------------------------------------------
constexpr int kChunk = 4;  // 128-k steps a wave requests at once

template <int MT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void nf4_stream_kernel(Nf4Args p) {
  __shared__ f32x4 red[WAVES][MT][64];
  __shared__ float tab[16];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kq = lane >> 4;
  if (threadIdx.x < 16) tab[threadIdx.x] = nf4_value(threadIdx.x);
  lds_barrier();
  const int n = blockIdx.x * 16 + (lane & 15);
  const int m0 = blockIdx.y * 16 * MT;
  const int ksteps = (p.K + 127) >> 7;
  const int ks0 = (ksteps * wave) / WAVES, ks1 = (ksteps * (wave + 1)) / WAVES;
  // columns past N read the last row (never stored); K % B == 0: row n's blocks start at n (K / B)
  const int nr = min(n, p.N - 1);
  const uint8_t* wrow = p.codes + (size_t)nr * (p.K >> 1);
  const int brow = nr * (p.K >> p.lb);
  const int kq32 = 32 * kq;
  const float mu = bf16_lo_to_f32(*p.mean);
  struct Stage {
    u32x4 c;
    int q;
    uint32_t f;
  };
  // (32 | K: the 32 k of a lane lie inside K or outside; outside, the row's first 32 are read and both operands zeroed)
  auto issue = [&](Stage (&st)[kChunk], int step) {
#pragma unroll
    for (int d = 0; d < kChunk; ++d) {
      const int k0 = (step + d) * 128 + kq32;
      const int kk = k0 < p.K ? k0 : 0;
      const int b = brow + (kk >> p.lb);
      st[d].c = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow + (kk >> 1)));
      st[d].q = p.q[b];
      st[d].f = p.qf[b >> p.lsb];
    }
    __builtin_amdgcn_sched_barrier(0);  // every request of the chunk is out before anything waits
  };
  // rows past M alias the tile's first row: they only reach outputs that are never stored
  size_t arow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = m0 + mt * 16 + (lane & 15);
    arow[mt] = (size_t)(row < p.M ? row : m0);
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
        const bool v = k0 < p.K;
        const u32x4 z = {0u, 0u, 0u, 0u};
        const float s = nf4_scaler(cur[d].q, bf16_lo_to_f32(cur[d].f), mu);
        u32x4 w[4];
        w[0] = nf4_decode8(cur[d].c.x, s, tab);
        w[1] = nf4_decode8(cur[d].c.y, s, tab);
        w[2] = nf4_decode8(cur[d].c.z, s, tab);
        w[3] = nf4_decode8(cur[d].c.w, s, tab);
        if (!v) w[0] = w[1] = w[2] = w[3] = z;  // (not 0 x scaler: a scaler may be NaN)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const u32x4* xp = reinterpret_cast<const u32x4*>(p.x + arow[mt] * p.K + (v ? k0 : 0));
          u32x4 a[4] = {xp[0], xp[1], xp[2], xp[3]};
          if (!v) a[0] = a[1] = a[2] = a[3] = z;
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
  for (int mt = wave; mt < MT; mt += WAVES) {
    f32x4 c = red[0][mt][lane];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) c += red[w][mt][lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + mt * 16 + 4 * kq + r;
      if (row < p.M && n < p.N) p.out[(size_t)row * p.N + n] = f32_to_bf16_bits(c[r]);
    }
  }
}

// (4 m-tiles x 16 waves: the meeting buffer would pass the static LDS; the stream-form plan caps 4 m-tiles at 8 waves)
int launch_stream(const TwoFormRoute& r, const Nf4Args& a, hipStream_t st) {
  return launch_stream_form<false>("nf4_stream_kernel", "nf4_stream_kernel launch", r, a, st,
                                   [](auto mt, auto waves) { return nf4_stream_kernel<decltype(mt)::value, decltype(waves)::value>; });
}

int check_format(const char* fn, int64_t numel, int64_t B, int64_t SB) {
  AO_REQUIRE(nf4_format_ok(numel, B, SB),
             "%s: bad format numel=%lld block_size=%lld scaler_block_size=%lld (block_size 32, 64 or 128, scaler_block_size a power of two, "
             "numel a multiple of block_size x scaler_block_size below 2^31)",
             fn, (long long)numel, (long long)B, (long long)SB);
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_nf4_block_absmax(const uint16_t* x, uint16_t* absmax, int64_t numel, int block_size, void* stream) {
  if (int rc = check_format(__func__, numel, block_size, 1)) return rc;
  if (numel == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(absmax);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(absmax, 2), "%s: x must be 16-byte, absmax 2-byte aligned", __func__);
  const int64_t pieces = numel / 8;
  ao::launch(nf4_absmax_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, absmax, pieces,
             log2_exact(block_size) - 3);
  AO_LAUNCH_CHECK("nf4_absmax_kernel launch");
  return AO_OK;
}

extern "C" int ao_nf4_quantize(const uint16_t* x, const uint16_t* absmax, const uint16_t* mean, uint8_t* codes, int8_t* scalers,
                               uint16_t* factors, int64_t numel, int block_size, int64_t scaler_block_size, void* stream) {
  if (int rc = check_format(__func__, numel, block_size, scaler_block_size)) return rc;
  if (numel == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(absmax);
  AO_REQUIRE_PTR(mean);
  AO_REQUIRE_PTR(codes);
  AO_REQUIRE_PTR(scalers);
  AO_REQUIRE_PTR(factors);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(codes, 4) && aligned_to(absmax, 2) && aligned_to(mean, 2) && aligned_to(factors, 2),
             "%s: x must be 16-byte, codes 4-byte, absmax, mean and factors 2-byte aligned", __func__);
  const int64_t pieces = numel / 8, scaler_blocks = numel / (block_size * scaler_block_size);
  const int64_t code_grid = (pieces + 255) / 256, grid = code_grid + (scaler_blocks + 3) / 4;
  AO_REQUIRE(grid < (1ll << 31), "%s: tensor too large for one launch", __func__);
  ao::launch(nf4_quantize_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), x, absmax, mean,
             reinterpret_cast<uint32_t*>(codes), scalers, factors, pieces, scaler_blocks, log2_exact(block_size), log2_exact(scaler_block_size),
             (unsigned)code_grid);
  AO_LAUNCH_CHECK("nf4_quantize_kernel launch");
  return AO_OK;
}

extern "C" int ao_nf4_dequantize(const uint8_t* codes, const int8_t* scalers, const uint16_t* factors, const uint16_t* mean, uint16_t* w,
                                 int64_t numel, int block_size, int64_t scaler_block_size, void* stream) {
  if (int rc = check_format(__func__, numel, block_size, scaler_block_size)) return rc;
  if (numel == 0) return AO_OK;
  AO_REQUIRE_PTR(codes);
  AO_REQUIRE_PTR(scalers);
  AO_REQUIRE_PTR(factors);
  AO_REQUIRE_PTR(mean);
  AO_REQUIRE_PTR(w);
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(codes, 4) && aligned_to(mean, 2) && aligned_to(factors, 2),
             "%s: w must be 16-byte, codes 4-byte, mean and factors 2-byte aligned", __func__);
  const int64_t pieces = numel / 8;
  ao::launch(nf4_dequantize_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
             reinterpret_cast<const uint32_t*>(codes), scalers, factors, mean, reinterpret_cast<u32x4*>(w), pieces, log2_exact(block_size),
             log2_exact(scaler_block_size));
  AO_LAUNCH_CHECK("nf4_dequantize_kernel launch");
  return AO_OK;
}

extern "C" int ao_nf4_linear_route(int64_t M, int64_t N, int64_t K, int block_size, int64_t scaler_block_size, int32_t* out, int cap) {
  return route_export(__func__, nf4_route(M, N, K, block_size, scaler_block_size), out, cap);
}

extern "C" const char* ao_nf4_linear_kernel_name(int64_t M, int64_t N, int64_t K, int block_size, int64_t scaler_block_size) {
  return nf4_route(M, N, K, block_size, scaler_block_size).kernel == 1 ? "nf4_stream_kernel" : "not fused";
}

extern "C" int ao_nf4_linear_set_form(int form) {
  AO_REQUIRE(form == 0 || form == 1, "%s: form must be 0 (route) or 1 (stream): there is no tiled form, got %d", __func__, form);
  return set_forced_form(__func__, form, g_form);
}

extern "C" int ao_nf4_linear(const uint16_t* x, const uint8_t* codes, const int8_t* scalers, const uint16_t* factors, const uint16_t* mean,
                             uint16_t* out, int64_t M, int64_t N, int64_t K, int block_size, int64_t scaler_block_size, void* stream) {
  AO_REQUIRE(nf4_linear_shape_ok(M, N, K, block_size, scaler_block_size),
             "%s: bad shape M=%lld N=%lld K=%lld block_size=%d scaler_block_size=%lld (M >= 0, N >= 1, block_size 32, 64 or 128 dividing K, "
             "scaler_block_size a power of two, N K a multiple of block_size x scaler_block_size, operands < 2^31 elements)",
             __func__, (long long)M, (long long)N, (long long)K, block_size, (long long)scaler_block_size);
  AO_REQUIRE_PTR(codes);
  AO_REQUIRE_PTR(scalers);
  AO_REQUIRE_PTR(factors);
  AO_REQUIRE_PTR(mean);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(codes, 16) && aligned_to(factors, 2) && aligned_to(mean, 2) && aligned_to(out, 2),
             "%s: x and codes must be 16-byte, factors, mean and out 2-byte aligned", __func__);
  const TwoFormRoute r = nf4_route(M, N, K, block_size, scaler_block_size);
  AO_REQUIRE(r.kernel == 1, "%s: M=%lld is not fused (more than %d rows, or more than 65535 grid rows): dequantize, then multiply", __func__,
             (long long)M, kStreamMaxRows);
  const Nf4Args args{x, codes, scalers, factors, mean, out, (int)M, (int)N, (int)K, log2_exact(block_size), log2_exact(scaler_block_size)};
  return launch_stream(r, args, static_cast<hipStream_t>(stream));
}
