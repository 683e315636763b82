// MX dense linears for gfx950: MXFP4 (e2m1) and MXFP8 (e4m3) elements with E8M0 scales over 1 x 32 blocks along K.
//
// Replaces the GEMM of torchao's MXTensor linear (prototype/mx_formats/mx_tensor.py:760-880, _addmm_mx_dispatch: F.scaled_mm with
// cuBLAS-swizzled scales under KernelPreference.AUTO, dequantise + aten mm / addmm under EMULATED) and the MXFP4 cast
// (to_mx(x, float4_e2m1fn_x2, 32, mode), :228-409).  The arithmetic:
//   out[m][n] = bf16( sum_k dq(a)[m][k] dq(b)[n][k] + bias[n] ),  dq = element 2^(scale - 127),
// fp32 accumulation in v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz / blgp = 4 for e2m1, 0 for e4m3), one rounding at the store.  The scales
// stay row-major [rows][K/32]: the scaled MFMA takes them as per-lane register operands, so no 128 x 4 swizzle is built or read.
//
// Operand lane map of the K = 128 scaled MFMA (lane l: row / column l & 15, lane group kq = l >> 4; its scale byte applies to 32-k block kq):
//   e4m3: lane group kq holds k = 16 kq .. +15 and 64 + 16 kq .. +15 (probed on gfx950, stream8_kernels.hip)
//   e2m1: lane group kq holds k = 32 kq .. +31 (four VGPRs, element 2i in the low nibble of byte i -- the packed layout of to_mx), so one
//         lane owns one whole block; tests/test_mx_linear_gpu.py pins this map with one-hot operands.
//
// Two forms, one route (mx_route: this family's shape check, seams and forced form over the plans of two_form_route.h)
// read by the launch and by ao_mx_linear_route / ao_mx_linear_kernel_name:
//   mx_linear_stream_kernel: the weight is streamed once; a workgroup owns 16 columns and splits K over its waves, the partial tiles
//     meet in LDS in wave order.  The bf16 activation may be cast inside (CAST): the lanes that feed the A operand cast their blocks with
//     the stand-alone casts' functions (quant_math.h: mx_cast4, mx_encode8), so the codes and scales are those of the cast kernels and
//     the result is bit-identical to cast + this kernel.  Up to 64 rows per workgroup (MT m-tiles of 16); more rows add grid rows
//     (forced forms only: the route hands e4m3 over at 64 rows, e2m1 at 32).
//   mx_linear_tile_kernel: 128 x 128 output tiles, four waves of 64 x 64, both operands staged in LDS by buffer_load ... lds (16 bytes a
//     lane), two stages; rows / columns past the matrix and k past K read as zero through the buffer's range check.
#include "common.h"
#include "quant_math.h"
#include "stream_blocks.h"
#include "two_form_route.h"

namespace ao {
namespace {

constexpr int kFmtE4M3 = AO_MX_FMT_E4M3;  // MFMA format codes (cbsz / blgp)
constexpr int kFmtE2M1 = AO_MX_FMT_E2M1;

// ---- the route ------------------------------------------------------------------------------------------------------------------
// Fitted on the Llama-3-8B five shapes (profiles/mx_linear_r07.jsonl, tools/bench_mx_linear.py --sweep, both forms forced at
// M = 1 .. 256): the streaming form up to these rows, the LDS-tiled form beyond -- the seams with the least summed time (e4m3 64: the
// five shapes at 64 rows take 264 us streamed, 438 us tiled; e2m1 32: gate / up at 32 rows 75 us streamed, 47 us tiled, qkv / o / down
// still ahead streamed).
constexpr int kStreamMaxRowsE4M3 = 64;
constexpr int kStreamMaxRowsE2M1 = 32;

thread_local int g_form = 0;  // ao_mx_linear_set_form: 0 the product route, 1 stream, 2 tile

bool mx_shape_ok(int fmt, int64_t M, int64_t N, int64_t K) {
  if (fmt != kFmtE4M3 && fmt != kFmtE2M1) return false;
  if (M < 0 || N < 1 || K < 32 || K % 32 != 0) return false;
  if (M >= (1ll << 31) || N >= (1ll << 31) || K >= (1ll << 31)) return false;
  const int64_t kb = fmt == kFmtE2M1 ? K / 2 : K;  // bytes per row of codes: the buffer ranges of the tile form are 32-bit
  return M * kb < (1ll << 31) && N * kb < (1ll << 31) && M * N < (1ll << 40);
}

// kernel 1: mx_linear_stream_kernel, 2: mx_linear_tile_kernel (128 x 128 tiles)
TwoFormRoute mx_route(int fmt, int64_t M, int64_t N, int64_t K) {
  if (!mx_shape_ok(fmt, M, N, K)) return TwoFormRoute{};
  const int seam = fmt == kFmtE2M1 ? kStreamMaxRowsE2M1 : kStreamMaxRowsE4M3;
  return two_form_route(g_form != 0 ? g_form : (M <= seam ? 1 : 2), M, N, K, 128);
}

struct MxArgs {
  const uint8_t* a;        // codes [M][K or K/2] (stream form without CAST, tile form)
  const uint8_t* a_scale;  // [M][K/32]
  const uint16_t* x;       // bf16 [M][K] (CAST)
  const uint8_t* b;        // codes [N][K or K/2]
  const uint8_t* b_scale;  // [N][K/32]
  const uint16_t* bias;    // bf16 [N] or null
  uint16_t* out;           // bf16 [M][N]
  int M, N, K;
};

__device__ __forceinline__ u32x4 ld16(const uint8_t* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ u32x4 ld16(const uint16_t* p) { return *reinterpret_cast<const u32x4*>(p); }

template <int FMT>
__device__ __forceinline__ f32x4 mx_mfma(const u32x4& a0, const u32x4& a1, const u32x4& b0, const u32x4& b1, f32x4 c, int sa, int sb) {
  return mfma8_k128<false, FMT>(a0, a1, b0, b1, c, sa, sb);
}

// One lane's operand of k step `step` for row `row` of a codes matrix (rows past `rows` and blocks past K read as zero, scale 127).
template <int FMT>
__device__ __forceinline__ void load_codes(const uint8_t* codes, const uint8_t* scales, int row, int rows, int step, int kq, int K,
                                           u32x4& v0, u32x4& v1, int& s) {
  const int kb = K >> 5;
  const bool rv = row < rows;
  v0 = u32x4{0u, 0u, 0u, 0u};
  v1 = v0;
  s = 127;
  if (FMT == kFmtE2M1) {
    const int blk = step * 4 + kq;
    if (rv && blk < kb) {
      v0 = ld16(codes + (size_t)row * (K >> 1) + blk * 16);
      s = scales[(size_t)row * kb + blk];
    }
  } else {
    const int k0 = step * 128 + 16 * kq;
    if (rv && k0 < K) v0 = ld16(codes + (size_t)row * K + k0);
    if (rv && k0 + 64 < K) v1 = ld16(codes + (size_t)row * K + k0 + 64);
    if (rv && step * 4 + kq < kb) s = scales[(size_t)row * kb + step * 4 + kq];
  }
}

// The same operand cast from the bf16 activation.  e4m3: the two halves of a lane belong to blocks step*4 + kq/2 and step*4 + 2 + kq/2,
// shared with lane l ^ 16; the scale byte of block kq is fetched from the lane that computed it.  Every lane runs the shuffles.
template <int FMT, int MODE>
__device__ __forceinline__ void cast_operand(const uint16_t* x, int row, int rows, int step, int lane, int K, u32x4& v0, u32x4& v1, int& s) {
  const int kq = lane >> 4, kb = K >> 5;
  const bool rv = row < rows;
  if (FMT == kFmtE2M1) {
    const int blk = step * 4 + kq;
    v1 = u32x4{0u, 0u, 0u, 0u};
    if (rv && blk < kb) {
      const uint16_t* p = x + (size_t)row * K + blk * 32;
      const u32x4 v[4] = {ld16(p), ld16(p + 8), ld16(p + 16), ld16(p + 24)};
      uint32_t e;
      v0 = mx_cast4<MODE>(v, e);
      s = (int)e;
    } else {
      v0 = v1;
      s = 127;
    }
  } else {
    const int k0 = step * 128 + 16 * kq;
    const u32x4 z = {0u, 0u, 0u, 0u};
    const bool lo = rv && k0 < K, hi = rv && k0 + 64 < K;
    const uint16_t* p = x + (size_t)row * K + k0;
    const u32x4 a0 = lo ? ld16(p) : z, a1 = lo ? ld16(p + 8) : z;
    const u32x4 a2 = hi ? ld16(p + 64) : z, a3 = hi ? ld16(p + 72) : z;
    bool nlo = false, nhi = false;
    float mlo = fmaxf(amax8(a0, nlo), amax8(a1, nlo));
    float mhi = fmaxf(amax8(a2, nhi), amax8(a3, nhi));
    mlo = fmaxf(mlo, __shfl_xor(mlo, 16));
    mhi = fmaxf(mhi, __shfl_xor(mhi, 16));
    const uint32_t flo = (nlo ? 1u : 0u) | (uint32_t)__shfl_xor((int)(nlo ? 1 : 0), 16);
    const uint32_t fhi = (nhi ? 1u : 0u) | (uint32_t)__shfl_xor((int)(nhi ? 1 : 0), 16);
    const uint32_t elo = mx_block_exponent<MODE>(mlo, flo == 0u && mlo < INFINITY);
    const uint32_t ehi = mx_block_exponent<MODE>(mhi, fhi == 0u && mhi < INFINITY);
    const u32x2 c0 = mx_encode8<MODE>(a0, elo), c1 = mx_encode8<MODE>(a1, elo);
    const u32x2 c2 = mx_encode8<MODE>(a2, ehi), c3 = mx_encode8<MODE>(a3, ehi);
    v0 = lo ? u32x4{c0.x, c0.y, c1.x, c1.y} : z;
    v1 = hi ? u32x4{c2.x, c2.y, c3.x, c3.y} : z;
    const int src = (lane & 15) + 16 * (kq < 2 ? 2 * kq : 2 * (kq - 2));
    const int slo = __shfl((int)elo, src), shi = __shfl((int)ehi, src);
    s = (rv && step * 4 + kq < kb) ? (kq < 2 ? slo : shi) : 127;
  }
}

// ---- streaming form -------------------------------------------------------------------------------------------------------------
template <int FMT, int CAST, int MT, int WAVES>  // CAST: 0 codes in, 1 floor, 2 rceil
__global__ __launch_bounds__(64 * WAVES) void mx_linear_stream_kernel(MxArgs p) {
  __shared__ f32x4 red[WAVES][MT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4;
  const int n = blockIdx.x * 16 + (lane & 15);
  const int m0 = blockIdx.y * 16 * MT;
  const int ksteps = (p.K + 127) >> 7;
  const int ks0 = (ksteps * wave) / WAVES, ks1 = (ksteps * (wave + 1)) / WAVES;
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int step = ks0; step < ks1; ++step) {
    u32x4 b0, b1;
    int sb;
    load_codes<FMT>(p.b, p.b_scale, n, p.N, step, kq, p.K, b0, b1, sb);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int row = m0 + mt * 16 + (lane & 15);
      u32x4 a0, a1;
      int sa;
      if constexpr (CAST == 0) load_codes<FMT>(p.a, p.a_scale, row, p.M, step, kq, p.K, a0, a1, sa);
      else cast_operand<FMT, CAST - 1>(p.x, row, p.M, step, lane, p.K, a0, a1, sa);
      acc[mt] = mx_mfma<FMT>(a0, a1, b0, b1, acc[mt], sa, sb);
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) red[wave][mt][lane] = acc[mt];
  __syncthreads();
  // wave w stores m-tiles w, w + WAVES, ...: the partial tiles are added in wave order
  const float bias = (p.bias != nullptr && n < p.N) ? bf16_lo_to_f32(p.bias[n]) : 0.f;
  for (int mt = wave; mt < MT; mt += WAVES) {
    f32x4 c = red[0][mt][lane];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) c += red[w][mt][lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + mt * 16 + 4 * kq + r;
      if (row < p.M && n < p.N) {
        float v = c[r];
        if (p.bias != nullptr) v += bias;
        p.out[(size_t)row * p.N + n] = f32_to_bf16_bits(v);
      }
    }
  }
}

// ---- LDS-tiled form -------------------------------------------------------------------------------------------------------------
// Stage layout: A then B, 128 rows each, RB bytes a row (128 e4m3 / 64 packed e2m1), 16-byte pieces swizzled by row so that the 16 lanes
// of a fragment read hit different banks: piece c of row r sits at slot r * PR + (c ^ (r % PR)).
template <int FMT>
struct TileCfg {
  static constexpr int RB = FMT == kFmtE2M1 ? 64 : 128;  // bytes a row a k step
  static constexpr int PR = RB / 16;                      // pieces a row
  static constexpr int OPB = 128 * RB;                    // bytes an operand a stage
  static constexpr int STAGE = 2 * OPB;
};

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, char* lds, uint32_t voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds, 16, voff, 0, 0, 0);
}

template <int FMT>
__device__ __forceinline__ void tile_issue(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb, char* stage, int m0, int n0, int step, int K,
                                           int wave, int lane) {
  using C = TileCfg<FMT>;
  const int rowbytes = FMT == kFmtE2M1 ? (K >> 1) : K;
  constexpr int kInstr = C::OPB / 1024;  // 1 KiB per wave instruction
#pragma unroll
  for (int i = wave; i < 2 * kInstr; i += 4) {
    const bool isb = i >= kInstr;
    const int j = isb ? i - kInstr : i;
    const int slot = j * 64 + lane;
    const int r = slot / C::PR, c = (slot % C::PR) ^ (r % C::PR);
    const int kbyte = step * C::RB + c * 16;
    const int grow = (isb ? n0 : m0) + r;
    const uint32_t voff = kbyte < rowbytes ? (uint32_t)grow * (uint32_t)rowbytes + (uint32_t)kbyte : 0xFFFFFFF0u;
    dma16(isb ? rb : ra, stage + (isb ? C::OPB : 0) + j * 1024, voff);
  }
}

template <int FMT>
__device__ __forceinline__ void tile_frag(const char* op, int r, int kq, u32x4& v0, u32x4& v1) {
  using C = TileCfg<FMT>;
  if (FMT == kFmtE2M1) {
    v0 = *reinterpret_cast<const u32x4*>(op + (r * C::PR + (kq ^ (r % C::PR))) * 16);
    v1 = u32x4{0u, 0u, 0u, 0u};
  } else {
    v0 = *reinterpret_cast<const u32x4*>(op + (r * C::PR + (kq ^ (r % C::PR))) * 16);
    v1 = *reinterpret_cast<const u32x4*>(op + (r * C::PR + ((kq + 4) ^ (r % C::PR))) * 16);
  }
}

__device__ __forceinline__ int scale_at(const uint8_t* scales, int row, int rows, int blk, int kb) {
  return (row < rows && blk < kb) ? (int)scales[(size_t)row * kb + blk] : 127;
}

template <int FMT>
__global__ __launch_bounds__(256) void mx_linear_tile_kernel(MxArgs p) {
  using C = TileCfg<FMT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4;
  const int m0 = blockIdx.y * 128, n0 = blockIdx.x * 128;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int rowbytes = FMT == kFmtE2M1 ? (p.K >> 1) : p.K;
  const int kb = p.K >> 5;
  // rows past the matrix fall outside the buffer's range and read as zero
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, 0, p.M * rowbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)p.b, 0, p.N * rowbytes, 0x00020000);
  const int ksteps = (p.K + 127) >> 7;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int sa[4], sb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sa[i] = scale_at(p.a_scale, m0 + wm + 16 * i + (lane & 15), p.M, kq, kb);
    sb[i] = scale_at(p.b_scale, n0 + wn + 16 * i + (lane & 15), p.N, kq, kb);
  }
  tile_issue<FMT>(ra, rb, smem, m0, n0, 0, p.K, wave, lane);
  for (int step = 0; step < ksteps; ++step) {
    char* cur = smem + (step & 1) * C::STAGE;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage `step` has landed for every wave; every wave is done with the other stage
    int na[4], nb[4];
    if (step + 1 < ksteps) {
      tile_issue<FMT>(ra, rb, smem + ((step + 1) & 1) * C::STAGE, m0, n0, step + 1, p.K, wave, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        na[i] = scale_at(p.a_scale, m0 + wm + 16 * i + (lane & 15), p.M, (step + 1) * 4 + kq, kb);
        nb[i] = scale_at(p.b_scale, n0 + wn + 16 * i + (lane & 15), p.N, (step + 1) * 4 + kq, kb);
      }
    }
    u32x4 bf0[4], bf1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) tile_frag<FMT>(cur + C::OPB, wn + 16 * j + (lane & 15), kq, bf0[j], bf1[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 a0, a1;
      tile_frag<FMT>(cur, wm + 16 * i + (lane & 15), kq, a0, a1);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mx_mfma<FMT>(a0, a1, bf0[j], bf1[j], acc[i][j], sa[i], sb[j]);
    }
    if (step + 1 < ksteps) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sa[i] = na[i];
        sb[i] = nb[i];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn + 16 * j + (lane & 15);
    if (n >= p.N) continue;
    const float bias = p.bias != nullptr ? bf16_lo_to_f32(p.bias[n]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + 16 * i + 4 * kq + r;
        if (row < p.M) {
          float v = acc[i][j][r];
          if (p.bias != nullptr) v += bias;
          p.out[(size_t)row * p.N + n] = f32_to_bf16_bits(v);
        }
      }
  }
}

// ---- the stand-alone MXFP4 cast: one lane per 32-block ----------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void mxfp4_quant_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ s,
                                                          int64_t blocks) {
  const int64_t blk = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (blk >= blocks) return;
  const uint16_t* p = x + blk * 32;
  const u32x4 v[4] = {ld16(p), ld16(p + 8), ld16(p + 16), ld16(p + 24)};
  uint32_t e;
  *reinterpret_cast<u32x4*>(q + blk * 16) = mx_cast4<MODE>(v, e);
  s[blk] = (uint8_t)e;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------
template <int FMT, int CAST>
int launch_stream(const TwoFormRoute& r, const MxArgs& a, hipStream_t st) {
  return launch_stream_form<true>("mx_linear_stream_kernel", "mx_linear_stream_kernel launch", r, a, st, [](auto mt, auto waves) {
    return mx_linear_stream_kernel<FMT, CAST, decltype(mt)::value, decltype(waves)::value>;
  });
}

template <int FMT>
int launch_tile(const TwoFormRoute& r, const MxArgs& a, hipStream_t st) {
  return launch_tile_form(mx_linear_tile_kernel<FMT>, "mx_linear_tile_kernel launch", r, a, st, 2 * TileCfg<FMT>::STAGE,
                          "hipFuncSetAttribute(mx_linear_tile_kernel)");
}

int check_linear(const char* fn, int fmt, int64_t M, int64_t N, int64_t K) {
  AO_REQUIRE(fmt == kFmtE4M3 || fmt == kFmtE2M1, "%s: fmt must be AO_MX_FMT_E4M3 (0) or AO_MX_FMT_E2M1 (4), got %d", fn, fmt);
  AO_REQUIRE(mx_shape_ok(fmt, M, N, K), "%s: bad shape M=%lld N=%lld K=%lld (M >= 0, N >= 1, K a positive multiple of 32, operands < 2 GiB)",
             fn, (long long)M, (long long)N, (long long)K);
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_mxfp4_quantize_rowwise(const uint16_t* x, uint8_t* q, uint8_t* scale_e8m0, int64_t R, int64_t C, int scaling_mode,
                                         void* stream) {
  AO_REQUIRE(R >= 0 && C > 0 && C % 32 == 0, "ao_mxfp4_quantize_rowwise: bad shape R=%lld C=%lld (C must be a positive multiple of 32)",
             (long long)R, (long long)C);
  AO_REQUIRE(scaling_mode == AO_MX_SCALE_FLOOR || scaling_mode == AO_MX_SCALE_RCEIL,
             "ao_mxfp4_quantize_rowwise: scaling_mode must be AO_MX_SCALE_FLOOR or AO_MX_SCALE_RCEIL, got %d", scaling_mode);
  if (R == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(scale_e8m0);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(q, 16), "ao_mxfp4_quantize_rowwise: x and q must be 16-byte aligned");
  const int64_t blocks = R * (C / 32);
  const int64_t grid = (blocks + 255) / 256;
  AO_REQUIRE(grid < (1ll << 31), "ao_mxfp4_quantize_rowwise: tensor too large for one launch");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (scaling_mode == AO_MX_SCALE_RCEIL)
    ao::launch(mxfp4_quant_kernel<AO_MX_SCALE_RCEIL>, dim3((unsigned)grid), dim3(256), 0, s, x, q, scale_e8m0, blocks);
  else
    ao::launch(mxfp4_quant_kernel<AO_MX_SCALE_FLOOR>, dim3((unsigned)grid), dim3(256), 0, s, x, q, scale_e8m0, blocks);
  AO_LAUNCH_CHECK("mxfp4_quant_kernel launch");
  return AO_OK;
}

extern "C" int ao_mx_linear_route(int fmt, int64_t M, int64_t N, int64_t K, int32_t* out, int cap) {
  return route_export(__func__, mx_route(fmt, M, N, K), out, cap);
}

extern "C" const char* ao_mx_linear_kernel_name(int fmt, int64_t M, int64_t N, int64_t K) {
  return route_kernel_name(mx_route(fmt, M, N, K), "mx_linear_stream_kernel", "mx_linear_tile_kernel");
}

extern "C" int ao_mx_linear_set_form(int form) { return set_forced_form(__func__, form, g_form); }

extern "C" int ao_mx_linear(int fmt, const uint8_t* a, const uint8_t* a_scale, const uint8_t* b, const uint8_t* b_scale, const uint16_t* bias,
                            uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream) {
  if (int rc = check_linear(__func__, fmt, M, N, K)) return rc;
  AO_REQUIRE_PTR(b);
  AO_REQUIRE_PTR(b_scale);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(a);
  AO_REQUIRE_PTR(a_scale);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(a, 16) && aligned_to(b, 16), "%s: the codes must be 16-byte aligned", __func__);
  const TwoFormRoute r = mx_route(fmt, M, N, K);
  AO_REQUIRE(r.kernel != 0, "%s: no route for M=%lld N=%lld K=%lld", __func__, (long long)M, (long long)N, (long long)K);
  const MxArgs args{a, a_scale, nullptr, b, b_scale, bias, out, (int)M, (int)N, (int)K};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (r.kernel == 1) return fmt == kFmtE2M1 ? launch_stream<kFmtE2M1, 0>(r, args, st) : launch_stream<kFmtE4M3, 0>(r, args, st);
  return fmt == kFmtE2M1 ? launch_tile<kFmtE2M1>(r, args, st) : launch_tile<kFmtE4M3>(r, args, st);
}

extern "C" int ao_mx_dynamic_linear_fits(int fmt, int64_t M, int64_t N, int64_t K) { return mx_route(fmt, M, N, K).kernel == 1 ? 1 : 0; }

extern "C" int ao_mx_dynamic_linear(int fmt, const uint16_t* x, const uint8_t* b, const uint8_t* b_scale, const uint16_t* bias, uint16_t* out,
                                    int64_t M, int64_t N, int64_t K, int scaling_mode, void* stream) {
  if (int rc = check_linear(__func__, fmt, M, N, K)) return rc;
  AO_REQUIRE(scaling_mode == AO_MX_SCALE_FLOOR || scaling_mode == AO_MX_SCALE_RCEIL,
             "%s: scaling_mode must be AO_MX_SCALE_FLOOR or AO_MX_SCALE_RCEIL, got %d", __func__, scaling_mode);
  AO_REQUIRE_PTR(b);
  AO_REQUIRE_PTR(b_scale);
  const TwoFormRoute r = mx_route(fmt, M, N, K);
  AO_REQUIRE(r.kernel == 1, "%s: M=%lld N=%lld K=%lld takes the tiled form: cast (ao_mx*_quantize_rowwise) and call ao_mx_linear", __func__,
             (long long)M, (long long)N, (long long)K);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(b, 16), "%s: x and the codes must be 16-byte aligned", __func__);
  const MxArgs args{nullptr, nullptr, x, b, b_scale, bias, out, (int)M, (int)N, (int)K};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool rceil = scaling_mode == AO_MX_SCALE_RCEIL;
  if (fmt == kFmtE2M1) return rceil ? launch_stream<kFmtE2M1, 2>(r, args, st) : launch_stream<kFmtE2M1, 1>(r, args, st);
  return rceil ? launch_stream<kFmtE4M3, 2>(r, args, st) : launch_stream<kFmtE4M3, 1>(r, args, st);
}
