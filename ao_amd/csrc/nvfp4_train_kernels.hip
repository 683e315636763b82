// NVFP4 training casts for gfx950: the operands of the three GEMMs of an NVFP4 linear (e2m1 codes, one e4m3 scale per block of 16, a
// per-tensor amax folded into the encode scale).
//
// Replaces, of torchao's prototype/moe_training/nvfp4_training: triton_rht_amax / cutedsl_rht_amax (hadamard_amax_triton.py),
// triton_rht_quantize_row_col / cutedsl_rht_quantize_row_col (hadamard_quantize_row_col_triton.py) and triton_weight_quantize_2d /
// cutedsl_weight_quantize_2d (quantize_2d_triton.py), which run on sm100 only.  The arithmetic contracts are stated once, in quant_math.h
// ("NVFP4 training").  Scales are written ROW-MAJOR, [rows][cols / 16], which is what the GEMMs of nvfp4_kernels.hip read; the reference's
// 128 x 4 swizzle exists for cuBLAS.
//
// One tile walk, nvfp4_train_cast_kernel<W2D, SR>: a workgroup of 256 threads owns a 128 x 128 tile of the bf16 source.
//   1. A thread loads four row blocks (16 consecutive elements of a row: 32 bytes; 8 adjacent lanes cover 256 contiguous bytes of a row),
//      keeps them in registers and stages them in LDS (rows 272 bytes apart); W2D also parks each row block's amax.
//   2. The ROW output is cast from the registers: a block's 8 bytes of codes and its scale byte leave directly, 8 adjacent lanes writing
//      64 contiguous bytes of a row of codes -- the tile's whole extent of that row.
//   3. The COLUMN output is the LDS transpose: a thread reads 16 consecutive rows of ONE column (lanes on adjacent columns: no bank
//      conflict), applies the randomized Hadamard transform (not W2D), casts, and stages 8 bytes of codes and a scale byte in a
//      transposed LDS tile, which then leaves as 64-byte runs of the transposed output, again the tile's whole extent of an output row.
//   W2D (the weight): both directions take the amax of the 16 x 16 block, the maximum of its 16 parked row-block amaxes, so the two outputs
//   hold the same block scales and the codes of the same values; no Hadamard transform, round to nearest even.
// Rows and columns past the matrix are guarded: they are staged as zeros and never stored.
// nvfp4_train_amax_kernel: a thread holds 16 rows x 2 adjacent columns (one dword a row, a wave 256 contiguous bytes), so both
// 16-point transforms stay in registers; one atomic max a workgroup and output over the non-negative bit patterns.
#include "common.h"
#include "quant_math.h"

#include <algorithm>

namespace ao {
namespace {

constexpr int kT = 128;                    // tile rows and columns
constexpr int kThreads = 256;
constexpr int kInStride = 2 * kT + 16;     // bytes between two rows of the staged bf16 tile (16-byte aligned row blocks)
constexpr int kOutStride = kT / 2 + 8;     // bytes between two columns of the staged transposed codes
constexpr int kUnits = kT * (kT / 16) / kThreads;  // blocks of 16 a thread casts per direction

struct TrainCastArgs {
  const uint16_t* x;        // bf16 [M][N]
  const float* amax_col;    // the per-tensor amax of the column output's values
  const float* amax_row;    // the per-tensor amax of the row output's values
  uint32_t sign_mask;       // bit i set: s_i = -1
  const int64_t* sr_seed;   // SR only
  const int64_t* col_offset;
  const int64_t* row_offset;
  uint8_t* col_q;           // [N][M/2] or null
  uint8_t* col_s;           // [N][M/16]
  uint8_t* row_q;           // [M][N/2] or null
  uint8_t* row_s;           // [M][N/16]
  int64_t M, N;
};

__device__ __forceinline__ void unpack16(const u32x4 (&v)[2], float (&a)[16]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[8 * i + 2 * j] = bf16_lo_to_f32(w[j]);
      a[8 * i + 2 * j + 1] = bf16_hi_to_f32(w[j]);
    }
  }
}

__device__ __forceinline__ float amax16(const float (&a)[16]) {
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) m = fmaxf(m, fabsf(a[i]));
  return m;
}

template <bool W2D, bool SR>
__global__ __launch_bounds__(kThreads) void nvfp4_train_cast_kernel(TrainCastArgs p) {
  __shared__ __attribute__((aligned(16))) uint8_t tin[kT * kInStride];
  __shared__ __attribute__((aligned(16))) uint8_t tout[kT * kOutStride];
  __shared__ uint8_t tsc[kT * 8];
  __shared__ float bam[W2D ? kT : 1][8];
  const int tid = threadIdx.x;
  const int64_t m0 = (int64_t)blockIdx.y * kT, n0 = (int64_t)blockIdx.x * kT;
  const bool do_row = p.row_q != nullptr, do_col = p.col_q != nullptr;
  uint32_t k0 = 0u, k1 = 0u, row_off = 0u, col_off = 0u;
  if (SR) {
    const uint64_t seed = (uint64_t)*p.sr_seed;
    k0 = (uint32_t)seed;
    k1 = (uint32_t)(seed >> 32);
    if (do_row) row_off = (uint32_t)(uint64_t)*p.row_offset;
    if (do_col) col_off = (uint32_t)(uint64_t)*p.col_offset;
  }
  // 1. the tile into registers and LDS
  u32x4 v[kUnits][2];
#pragma unroll
  for (int u = 0; u < kUnits; ++u) {
    const int id = u * kThreads + tid, r = id >> 3, cb = id & 7;
    const int64_t gm = m0 + r, gn = n0 + 16 * cb;
    const u32x4 z = {0u, 0u, 0u, 0u};
    v[u][0] = v[u][1] = z;
    if (gm < p.M && gn < p.N) {  // (16 | N: a block lies inside or outside)
      const u32x4* px = reinterpret_cast<const u32x4*>(p.x + gm * p.N + gn);
      v[u][0] = px[0];
      v[u][1] = px[1];
    }
    if (do_col) {
      u32x4* dst = reinterpret_cast<u32x4*>(tin + r * kInStride + cb * 32);
      dst[0] = v[u][0];
      dst[1] = v[u][1];
    }
    if constexpr (W2D) {
      bool has_nan = false;
      bam[r][cb] = fmaxf(amax8(v[u][0], has_nan), amax8(v[u][1], has_nan));
    }
  }
  if (W2D || do_col) __syncthreads();
  // 2. the row output, from the registers
  if (do_row) {
    const Nvfp4TrainGlobal gl = nvfp4_train_global(*p.amax_row);
#pragma unroll
    for (int u = 0; u < kUnits; ++u) {
      const int id = u * kThreads + tid, r = id >> 3, cb = id & 7;
      const int64_t gm = m0 + r, gn = n0 + 16 * cb;
      if (gm < p.M && gn < p.N) {
        float a[16];
        unpack16(v[u], a);
        float bm;
        if constexpr (W2D) {
          bm = 0.f;
#pragma unroll
          for (int i = 0; i < 16; ++i) bm = fmaxf(bm, bam[(r & ~15) + i][cb]);
        } else {
          bm = amax16(a);
        }
        uint32_t s8;
        const float enc = nvfp4_train_encode(bm, gl, s8);
        const u32x2 q = nvfp4_train_codes16<SR>(a, enc, (uint64_t)(gm * p.N + gn) >> 3, row_off, 0u, k0, k1);
        *reinterpret_cast<u32x2*>(p.row_q + gm * (p.N >> 1) + (gn >> 1)) = q;
        p.row_s[gm * (p.N >> 4) + (gn >> 4)] = (uint8_t)s8;
      }
    }
  }
  if (!do_col) return;  // (workgroup-uniform)
  // 3. the column output: 16 rows of one column a thread, staged transposed
  const Nvfp4TrainGlobal gl = nvfp4_train_global(*p.amax_col);
#pragma unroll
  for (int u = 0; u < kUnits; ++u) {
    const int id = u * kThreads + tid, c = id & (kT - 1), mb = id >> 7;
    const int64_t gn = n0 + c, gm = m0 + 16 * mb;
    if (gn < p.N && gm < p.M) {  // (16 | M)
      float a[16];
#pragma unroll
      for (int i = 0; i < 16; ++i)
        a[i] = bf16_lo_to_f32(*reinterpret_cast<const uint16_t*>(tin + (16 * mb + i) * kInStride + 2 * c));
      float bm;
      if constexpr (W2D) {
        bm = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) bm = fmaxf(bm, bam[16 * mb + i][c >> 4]);
      } else {
        nvfp4_rht16(a, p.sign_mask);
        bm = amax16(a);
      }
      uint32_t s8;
      const float enc = nvfp4_train_encode(bm, gl, s8);
      const u32x2 q = nvfp4_train_codes16<SR>(a, enc, (uint64_t)(gn * p.M + gm) >> 3, col_off, 1u, k0, k1);
      *reinterpret_cast<u32x2*>(tout + c * kOutStride + mb * 8) = q;
      tsc[c * 8 + mb] = (uint8_t)s8;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kUnits; ++u) {
    const int id = u * kThreads + tid, c = id >> 3, mb = id & 7;
    const int64_t gn = n0 + c, gm = m0 + 16 * mb;
    if (gn < p.N && gm < p.M) {
      *reinterpret_cast<u32x2*>(p.col_q + gn * (p.M >> 1) + (gm >> 1)) = *reinterpret_cast<const u32x2*>(tout + c * kOutStride + mb * 8);
      p.col_s[gn * (p.M >> 4) + (gm >> 4)] = tsc[c * 8 + mb];
    }
  }
}

__global__ void nvfp4_train_amax_clear_kernel(uint32_t* out2) {
  if (threadIdx.x < 2) out2[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(kThreads) void nvfp4_train_amax_kernel(const uint16_t* __restrict__ x, int64_t M, int64_t N, uint32_t sign_mask,
                                                                    int want_rht, uint32_t* out2) {
  const int64_t half = N >> 1, units = (M >> 4) * half;
  const uint32_t* px = reinterpret_cast<const uint32_t*>(x);
  float mr = 0.f, mc = 0.f;
  for (int64_t unit = (int64_t)blockIdx.x * kThreads + threadIdx.x; unit < units; unit += (int64_t)gridDim.x * kThreads) {
    const int64_t mb = unit / half, c2 = unit - mb * half;
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
  // one atomic a workgroup and output, not one a wave: 1024 workgroups then queue 1024 atomics on each of the two addresses, not 4096
  __shared__ float red[2][kThreads / 64];
  mr = wave_max(mr);
  mc = wave_max(mc);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mc;
    red[1][threadIdx.x >> 6] = mr;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    float m = 0.f;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) m = fmaxf(m, red[threadIdx.x][w]);
    if (m > 0.f) atomicMax(out2 + threadIdx.x, f32_to_bits(m));  // (cleared to 0: nothing to add otherwise)
  }
}

int check_mn(const char* fn, int64_t M, int64_t N) {
  AO_REQUIRE(M >= 0 && N > 0 && M % 16 == 0 && N % 16 == 0 && M < (1ll << 31) && N < (1ll << 31) && M * N < (1ll << 40),
             "%s: bad shape %lld x %lld (both multiples of 16, columns > 0, each below 2^31 and the product below 2^40)", fn, (long long)M,
             (long long)N);
  return AO_OK;
}

// the three instances that have a caller: the activation cast under either rounding, the weight cast under round to nearest even
template <bool W2D, bool SR>
int launch_cast(const TrainCastArgs& a, hipStream_t st) {
  static_assert(!(W2D && SR), "the weight is never rounded stochastically");
  const dim3 grid((unsigned)((a.N + kT - 1) / kT), (unsigned)((a.M + kT - 1) / kT));
  ao::launch(nvfp4_train_cast_kernel<W2D, SR>, grid, dim3(kThreads), 0, st, a);
  AO_LAUNCH_CHECK("nvfp4_train_cast_kernel launch");
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_nvfp4_train_amax(const uint16_t* x, float* out2, int64_t M, int64_t N, uint32_t sign_mask, int want_rht, void* stream) {
  if (int rc = check_mn(__func__, M, N)) return rc;
  AO_REQUIRE(sign_mask < (1u << 16), "%s: sign_mask must be a 16-bit mask, got 0x%x", __func__, sign_mask);
  AO_REQUIRE_PTR(out2);
  AO_REQUIRE(aligned_to(out2, 4), "%s: out2 must be 4-byte aligned", __func__);
  if (M > 0) {
    AO_REQUIRE_PTR(x);
    AO_REQUIRE(aligned_to(x, 16), "%s: x must be 16-byte aligned", __func__);
  }
  // every check is above: nothing is launched for a call that is refused
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* bits = reinterpret_cast<uint32_t*>(out2);
  ao::launch(nvfp4_train_amax_clear_kernel, dim3(1), dim3(64), 0, s, bits);
  if (M > 0) {
    const int64_t units = (M / 16) * (N / 2);
    const int64_t grid = std::min<int64_t>((units + kThreads - 1) / kThreads, 1024);
    ao::launch(nvfp4_train_amax_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, x, M, N, sign_mask, want_rht, bits);
  }
  AO_LAUNCH_CHECK("nvfp4_train_amax kernels launch");
  return AO_OK;
}

extern "C" int ao_nvfp4_train_quantize_row_col(const uint16_t* x, const float* amax2, uint32_t sign_mask, const int64_t* sr_seed,
                                               const int64_t* col_offset, const int64_t* row_offset, uint8_t* col_q, uint8_t* col_s, uint8_t* row_q,
                                               uint8_t* row_s, int64_t M, int64_t N, void* stream) {
  if (int rc = check_mn(__func__, M, N)) return rc;
  AO_REQUIRE(sign_mask < (1u << 16), "%s: sign_mask must be a 16-bit mask, got 0x%x", __func__, sign_mask);
  AO_REQUIRE((col_q == nullptr) == (col_s == nullptr) && (row_q == nullptr) == (row_s == nullptr),
             "%s: an output's codes and scales are given together or both null", __func__);
  AO_REQUIRE(col_q != nullptr || row_q != nullptr, "%s: both outputs are null", __func__);
  AO_REQUIRE_PTR(amax2);
  if (sr_seed != nullptr) {
    if (col_q != nullptr) AO_REQUIRE_PTR(col_offset);
    if (row_q != nullptr) AO_REQUIRE_PTR(row_offset);
  }
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(col_q, 8) && aligned_to(row_q, 8) && aligned_to(amax2, 4) && aligned_to(sr_seed, 8) &&
                 aligned_to(col_offset, 8) && aligned_to(row_offset, 8),
             "%s: x must be 16-byte, the codes, the seed and the offsets 8-byte and amax2 4-byte aligned", __func__);
  const TrainCastArgs a{x, amax2, amax2 + 1, sign_mask, sr_seed, col_offset, row_offset, col_q, col_s, row_q, row_s, M, N};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return sr_seed != nullptr ? launch_cast<false, true>(a, st) : launch_cast<false, false>(a, st);
}

extern "C" int ao_nvfp4_train_quantize_weight_2d(const uint16_t* w, const float* amax, uint8_t* q, uint8_t* s, uint8_t* qt, uint8_t* st, int64_t N,
                                                 int64_t K, void* stream) {
  if (int rc = check_mn(__func__, N, K)) return rc;
  AO_REQUIRE_PTR(amax);
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(s);
  AO_REQUIRE_PTR(qt);
  AO_REQUIRE_PTR(st);
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(q, 8) && aligned_to(qt, 8) && aligned_to(amax, 4),
             "%s: w must be 16-byte, the codes 8-byte and amax 4-byte aligned", __func__);
  const TrainCastArgs a{w, amax, amax, 0u, nullptr, nullptr, nullptr, qt, st, q, s, N, K};
  return launch_cast<true, false>(a, static_cast<hipStream_t>(stream));
}
