// Tiled MFMA GEMM for 1-byte operands on gfx950: y = epilogue(A[M,K] @ B[N,K]^T)
//   * int8 x int8 -> int32  (aten::_int_mm / the Int8Tensor linear:
//     torchao/quantization/quantize_/workflows/int8/kernels.py:114-144,
//     int8_tensor.py:305-359) on v_mfma_i32_32x32x32_i8
//   * e4m3 x e4m3 -> fp32   (aten::_scaled_mm rowwise, torchao/float8/inference.py:
//     86-123) on v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales (the
//     K=64 form is the only full-rate fp8 path on CDNA4)
// Both operands are K-contiguous ("NT"), so A and B tiles are staged the same
// way: 128 x 128-byte tiles, 16 B per thread per pass, through padded LDS rows
// (144 B stride: ds_read_b128 conflict-free), double buffered, one barrier per
// K step.  4 waves as 2x2, each 64x64 = 2x2 MFMA tiles of 32x32.
// The epilogue applies the reference's scaling sequence in registers and stores
// bf16 (or raw int32 for _int_mm).
#include "common.h"
#include "gemm8_route.h"
#include "quant_math.h"

namespace ao {
// the launchers: each takes the launch shape gemm8_route picked (epi numbering of gemm8_p8 / gemm8_p8h = enum Epilogue)
int gemm8_p8(int epi, const uint8_t* a, const uint8_t* b, const float* row_scale, const float* col_scale, const uint16_t* bias, void* out,
             int64_t M, int64_t N, int64_t K, bool persistent, hipStream_t stream);  // gemm8_p8_kernels.hip
int gemm8_p8h(int epi, const uint8_t* a, const uint8_t* b, const float* row_scale, const float* col_scale, const uint16_t* bias, void* out,
              int64_t M, int64_t N, int64_t K, int split, hipStream_t stream);
int rb8_scaled(bool int8, const void* a, const void* b, const float* scale_a, const float* scale_b, const uint16_t* bias, uint16_t* y, int64_t M,
               int64_t N, int64_t K, int bm, int bn, int split, hipStream_t stream);  // rb8_kernels.hip
int mid8_scaled(bool int8, const void* a, const float* scale_a, const void* b, const float* scale_b, const uint16_t* bias, uint16_t* y, int64_t M,
                int64_t N, int64_t K, const Mid8Plan& plan, hipStream_t stream);  // mid8_kernels.hip
int dec8_scaled(bool int8, const void* xq, const float* x_scale, const void* wq, const float* w_scale, const uint16_t* bias, uint16_t* y,
                int64_t M, int64_t N, int64_t K, const Dec8Shape& s, hipStream_t stream);  // dec8_kernels.hip
int int8_scaled_stream(const int8_t* a, const int8_t* b, const float* scale_a, const float* scale_b, const uint16_t* bias, uint16_t* y,
                       int64_t M, int64_t N, int64_t K, hipStream_t stream);
int fp8_rowwise_stream(const uint8_t* a, const uint8_t* b, const float* scale_a, const float* scale_b,
                       const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K, hipStream_t stream);

namespace {


constexpr int BM = 128, BN = 128, BK = 128;  // BK in bytes == elements
constexpr int LDS_STRIDE = BK + 16;          // 144 B
constexpr int TILE_BYTES = BM * LDS_STRIDE;  // one operand tile
constexpr int THREADS = 256;

// EPI_FP8_RAW: the unscaled fp32 accumulators (K-sharded row-parallel linears all-reduce them before the scale epilogue)
enum Epilogue { EPI_INT8_SCALED = 0, EPI_INT32 = 1, EPI_FP8_ROWWISE = 2, EPI_FP8_RAW = 3 };

struct Gemm8Args {
  const uint8_t* a;  // [M][K]
  const uint8_t* b;  // [N][K]
  const float* row_scale;  // [M]
  const float* col_scale;  // [N]
  const uint16_t* bias;    // [N] bf16 or null
  void* out;               // bf16 [M][N] or int32 [M][N]
  int M, N, K;
};

template <int EPI>
struct Acc {
  using type = f32x16;
};
template <>
struct Acc<EPI_INT8_SCALED> {
  using type = i32x16;
};
template <>
struct Acc<EPI_INT32> {
  using type = i32x16;
};

template <int EPI>
__global__ __launch_bounds__(THREADS) void gemm8_kernel(Gemm8Args p) {
  constexpr bool IS_INT = (EPI != EPI_FP8_ROWWISE && EPI != EPI_FP8_RAW);
  using acc_t = typename Acc<EPI>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 bufs][A tile | B tile]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;

  // global -> register staging: 4 passes x 16 B per operand per thread
  // chunk c = pass * 256 + tid: row = c >> 3 (8 chunks per 128-B row), col16 = c & 7
  const int srow = tid >> 3, scol = (tid & 7) * 16;
  const uint8_t* ag[4];
  const uint8_t* bg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = srow + i * 32;
    ag[i] = p.a + (size_t)min(m0 + r, p.M - 1) * p.K + scol;
    bg[i] = p.b + (size_t)min(n0 + r, p.N - 1) * p.K + scol;
  }
  const int ktiles = (p.K + BK - 1) / BK;

  u32x4 ra[4], rb[4];
  auto gload = [&](int kt) {
    const int k = kt * BK + scol;
    const bool in = (k + 16 <= p.K);  // K % 16 == 0: a chunk is entirely in or out
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = in ? *reinterpret_cast<const u32x4*>(ag[i] + (size_t)kt * BK) : u32x4{0, 0, 0, 0};
      rb[i] = in ? *reinterpret_cast<const u32x4*>(bg[i] + (size_t)kt * BK) : u32x4{0, 0, 0, 0};
    }
  };
  auto lstore = [&](int buf) {
    char* base = smem + buf * 2 * TILE_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = (srow + i * 32) * LDS_STRIDE + scol;
      *reinterpret_cast<u32x4*>(base + off) = ra[i];
      *reinterpret_cast<u32x4*>(base + TILE_BYTES + off) = rb[i];
    }
  };

  acc_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

  // fragment addressing: row = lane & 31 of the 32-row tile, 32 bytes at (lane >> 5) * 32 of each 64-byte chunk
  const int frow = lane & 31, fk = (lane >> 5) * 32;

  gload(0);
  lstore(0);
  __syncthreads();

  for (int kt = 0; kt < ktiles; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < ktiles) gload(kt + 1);
    const char* abase = smem + buf * 2 * TILE_BYTES + (wm * 64 + frow) * LDS_STRIDE + fk;
    const char* bbase = smem + buf * 2 * TILE_BYTES + TILE_BYTES + (wn * 64 + frow) * LDS_STRIDE + fk;
#pragma unroll
    for (int kc = 0; kc < BK / 64; ++kc) {
      u32x4 af[2][2], bf[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i][0] = *reinterpret_cast<const u32x4*>(abase + i * 32 * LDS_STRIDE + kc * 64);
        af[i][1] = *reinterpret_cast<const u32x4*>(abase + i * 32 * LDS_STRIDE + kc * 64 + 16);
        bf[i][0] = *reinterpret_cast<const u32x4*>(bbase + i * 32 * LDS_STRIDE + kc * 64);
        bf[i][1] = *reinterpret_cast<const u32x4*>(bbase + i * 32 * LDS_STRIDE + kc * 64 + 16);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr (IS_INT) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const i32x4 av = {(int)af[i][h].x, (int)af[i][h].y, (int)af[i][h].z, (int)af[i][h].w};
              const i32x4 bv = {(int)bf[j][h].x, (int)bf[j][h].y, (int)bf[j][h].z, (int)bf[j][h].w};
              acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc[i][j], 0, 0, 0);
            }
          } else {
            const i32x8 av = {(int)af[i][0].x, (int)af[i][0].y, (int)af[i][0].z, (int)af[i][0].w,
                              (int)af[i][1].x, (int)af[i][1].y, (int)af[i][1].z, (int)af[i][1].w};
            const i32x8 bv = {(int)bf[j][0].x, (int)bf[j][0].y, (int)bf[j][0].z, (int)bf[j][0].w,
                              (int)bf[j][1].x, (int)bf[j][1].y, (int)bf[j][1].z, (int)bf[j][1].w};
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[i][j], 0, 0, 0, 127, 0, 127);
          }
        }
    }
    if (kt + 1 < ktiles) lstore(buf ^ 1);
    __syncthreads();
  }

  // epilogue: C layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gn = n0 + wn * 64 + j * 32 + (lane & 31);
      if (gn >= p.N) continue;
      float cs = 1.f, bias = 0.f;
      if (EPI != EPI_INT32 && EPI != EPI_FP8_RAW) {
        cs = p.col_scale[gn];
        if (p.bias != nullptr) bias = bf16_lo_to_f32(p.bias[gn]);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (gm >= p.M) continue;
        if (EPI == EPI_INT32) {
          reinterpret_cast<int32_t*>(p.out)[(size_t)gm * p.N + gn] = (int32_t)acc[i][j][r];
        } else if (EPI == EPI_FP8_RAW) {
          reinterpret_cast<float*>(p.out)[(size_t)gm * p.N + gn] = (float)acc[i][j][r];
        } else {
          const float y = epilogue8<EPI == EPI_INT8_SCALED>((float)acc[i][j][r], p.row_scale[gm], cs, p.bias != nullptr, bias);
          reinterpret_cast<uint16_t*>(p.out)[(size_t)gm * p.N + gn] = f32_to_bf16_bits(y);
        }
      }
    }
}

// ---------------------------------------------------------------------------------------------
// The same GEMM with LDS-DMA staging (global_load_lds_dwordx4: 1 KiB per wave instruction straight
// into LDS, no VGPR round trip, no ds_write pass) -- the single biggest step of the CDNA4 GEMM ladder
// for this two-barrier structure.  LDS-DMA writes lane-linear, so rows cannot be padded; bank
// conflicts of the fragment reads are removed by a swizzle applied on the SOURCE address instead:
// LDS[row][chunk'] holds global 16-byte chunk  chunk' ^ f(row),  f(row) = (row & 7) ^ ((row >> 3) & 7)
// (within the 16 rows of every ds_read_b128 lane group, f is a bijection per row parity -> 16
// distinct 16-byte bank slots).  Needs K % 128 == 0; ragged M/N rows are clamped (never stored).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void dma16(const void* gsrc, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ int swz(int row) { return (row & 7) ^ ((row >> 3) & 7); }

// TM = 32-row MFMA tiles per wave along M: wave tile (TM*32) x 64, workgroup tile (TM*64) x 128.
// At TM = 2 every K step moves 64 KiB from LDS per CU for 512 MFMA cycles per SIMD -- LDS time equals
// MFMA time; TM = 4 (256 x 128 workgroup tile, 128 accumulator registers per lane) does 1024 MFMA
// cycles per 96 KiB of LDS reads.
// WN = waves along n (2: 4-wave workgroup, 128 columns; 4: 8-wave workgroup, 256 columns -- with TM = 4 the
// 256 x 256 tile whose wave tile is 128 x 64 (LDS reads 24 B per MFMA cycle instead of 32) at two waves per SIMD).
// TNJ = 32-column MFMA tiles per wave along N (2 or 4).
template <int EPI, int TM, int WN, int TNJ = 2>
__global__ __launch_bounds__(128 * WN) void gemm8_dma_kernel(Gemm8Args p) {
  constexpr bool IS_INT = (EPI != EPI_FP8_ROWWISE && EPI != EPI_FP8_RAW);
  constexpr int NWAVES = 2 * WN;
  constexpr int WGM = TM * 64;            // workgroup rows
  constexpr int WGN = WN * TNJ * 32;      // workgroup columns
  constexpr int A_TILE = WGM * BK;        // bytes, unpadded
  constexpr int B_TILE = WGN * BK;
  constexpr int A_DMAS = WGM / 8 / NWAVES;  // 1 KiB DMA instructions (8 rows each) per wave for the A tile
  constexpr int B_DMAS = WGN / 8 / NWAVES;
  using acc_t = typename Acc<EPI>::type;
  extern __shared__ __attribute__((aligned(1024))) char smem[];  // [2 bufs][A tile | B tile]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = blockIdx.y * WGM, n0 = blockIdx.x * WGN;
  const int ktiles = p.K / BK;
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(smem));

  // DMA sources: wave w fills rows (w*A_DMAS + i)*8 .. +7 of the A tile (and (w*B_DMAS + i)*8 of the B tile);
  // lane l lands at row r0 + (l >> 3), position l & 7 -> it must fetch chunk (l & 7) ^ f(row)
  const uint8_t* asrc[A_DMAS];
  const uint8_t* bsrc[B_DMAS];
#pragma unroll
  for (int i = 0; i < A_DMAS; ++i) {
    const int row = (wave * A_DMAS + i) * 8 + (lane >> 3);
    asrc[i] = p.a + (size_t)min(m0 + row, p.M - 1) * p.K + (((lane & 7) ^ swz(row)) << 4);
  }
#pragma unroll
  for (int i = 0; i < B_DMAS; ++i) {
    const int row = (wave * B_DMAS + i) * 8 + (lane >> 3);
    bsrc[i] = p.b + (size_t)min(n0 + row, p.N - 1) * p.K + (((lane & 7) ^ swz(row)) << 4);
  }
  auto stage = [&](int kt, int buf) {
    const uint32_t abase = lds0 + buf * (A_TILE + B_TILE);
#pragma unroll
    for (int i = 0; i < A_DMAS; ++i) dma16(asrc[i] + (size_t)kt * BK, abase + (wave * A_DMAS + i) * 1024);
#pragma unroll
    for (int i = 0; i < B_DMAS; ++i) dma16(bsrc[i] + (size_t)kt * BK, abase + A_TILE + (wave * B_DMAS + i) * 1024);
  };

  acc_t acc[TM][TNJ];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TNJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

  // fragment addressing: row = lane & 31 of the 32-row MFMA tile, logical chunks (lane >> 5) * 2 + {0, 1} of each
  // 64-byte k-slice; physical chunk = logical ^ f(row)
  const int frow = lane & 31, fc = (lane >> 5) * 2;
  int arow_off[TM], asw[TM], brow_off[TNJ], bsw[TNJ];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int ra = wm * (TM * 32) + i * 32 + frow;
    arow_off[i] = ra * BK; asw[i] = swz(ra);
  }
#pragma unroll
  for (int j = 0; j < TNJ; ++j) {
    const int rb = wn * (TNJ * 32) + j * 32 + frow;
    brow_off[j] = rb * BK; bsw[j] = swz(rb);
  }

  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");

  for (int kt = 0; kt < ktiles; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < ktiles) stage(kt + 1, buf ^ 1);
    const char* abase = smem + buf * (A_TILE + B_TILE);
    const char* bbase = abase + A_TILE;
#pragma unroll
    for (int kc = 0; kc < BK / 64; ++kc) {
      u32x4 af[TM][2], bf[TNJ][2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = kc * 4 + fc + h;
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i][h] = *reinterpret_cast<const u32x4*>(abase + arow_off[i] + ((c ^ asw[i]) << 4));
#pragma unroll
        for (int j = 0; j < TNJ; ++j) bf[j][h] = *reinterpret_cast<const u32x4*>(bbase + brow_off[j] + ((c ^ bsw[j]) << 4));
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TNJ; ++j) {
          if constexpr (IS_INT) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const i32x4 av = {(int)af[i][h].x, (int)af[i][h].y, (int)af[i][h].z, (int)af[i][h].w};
              const i32x4 bv = {(int)bf[j][h].x, (int)bf[j][h].y, (int)bf[j][h].z, (int)bf[j][h].w};
              acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc[i][j], 0, 0, 0);
            }
          } else {
            const i32x8 av = {(int)af[i][0].x, (int)af[i][0].y, (int)af[i][0].z, (int)af[i][0].w,
                              (int)af[i][1].x, (int)af[i][1].y, (int)af[i][1].z, (int)af[i][1].w};
            const i32x8 bv = {(int)bf[j][0].x, (int)bf[j][0].y, (int)bf[j][0].z, (int)bf[j][0].w,
                              (int)bf[j][1].x, (int)bf[j][1].y, (int)bf[j][1].z, (int)bf[j][1].w};
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[i][j], 0, 0, 0, 127, 0, 127);
          }
        }
    }
    // next tile landed (this wave's DMAs) and everybody is done reading `buf`
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }

  // epilogue: C layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TNJ; ++j) {
      const int gn = n0 + wn * (TNJ * 32) + j * 32 + (lane & 31);
      if (gn >= p.N) continue;
      float cs = 1.f, bias = 0.f;
      if (EPI != EPI_INT32 && EPI != EPI_FP8_RAW) {
        cs = p.col_scale[gn];
        if (p.bias != nullptr) bias = bf16_lo_to_f32(p.bias[gn]);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wm * (TM * 32) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (gm >= p.M) continue;
        if (EPI == EPI_INT32) {
          reinterpret_cast<int32_t*>(p.out)[(size_t)gm * p.N + gn] = (int32_t)acc[i][j][r];
        } else if (EPI == EPI_FP8_RAW) {
          reinterpret_cast<float*>(p.out)[(size_t)gm * p.N + gn] = (float)acc[i][j][r];
        } else {
          const float y = epilogue8<EPI == EPI_INT8_SCALED>((float)acc[i][j][r], p.row_scale[gm], cs, p.bias != nullptr, bias);
          reinterpret_cast<uint16_t*>(p.out)[(size_t)gm * p.N + gn] = f32_to_bf16_bits(y);
        }
      }
    }
}

template <int EPI, int TM, int WN, int TNJ = 2>
int launch_gemm8_dma(const Gemm8Args& p, hipStream_t stream) {
  constexpr int WGM = TM * 64, WGN = WN * TNJ * 32;
  dim3 grid((unsigned)((p.N + WGN - 1) / WGN), (unsigned)((p.M + WGM - 1) / WGM)), block(128 * WN);
  const size_t smem = 2 * (size_t)(WGM + WGN) * BK;  // 64 KiB (128 x 128) ... 128 KiB (256 x 256)
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(gemm8_dma_kernel<EPI, TM, WN, TNJ>), smem, "hipFuncSetAttribute(gemm8_dma_kernel)")) return rc;
  ao::launch(gemm8_dma_kernel<EPI, TM, WN, TNJ>, grid, block, smem, stream, p);
  AO_LAUNCH_CHECK("gemm8_dma_kernel launch");
  return AO_OK;
}

// the tiled GEMMs: the kernel of a route that reached the tiled forms
template <int EPI>
int launch_gemm8(const Gemm8Route& r, const Gemm8Args& p, hipStream_t stream) {
  switch (r.kernel) {
    case Gemm8Kernel::Dma128: return launch_gemm8_dma<EPI, 2, 2>(p, stream);
    case Gemm8Kernel::Dma256: return launch_gemm8_dma<EPI, 4, 4>(p, stream);
    case Gemm8Kernel::Dma256x128: return launch_gemm8_dma<EPI, 4, 2>(p, stream);
    case Gemm8Kernel::Dma256x256w4: return launch_gemm8_dma<EPI, 4, 2, 4>(p, stream);
    case Gemm8Kernel::P8h: return gemm8_p8h((int)EPI, p.a, p.b, p.row_scale, p.col_scale, p.bias, p.out, p.M, p.N, p.K, r.k_parts, stream);
    case Gemm8Kernel::P8:
    case Gemm8Kernel::P8p:
      return gemm8_p8((int)EPI, p.a, p.b, p.row_scale, p.col_scale, p.bias, p.out, p.M, p.N, p.K, r.kernel == Gemm8Kernel::P8p, stream);
    case Gemm8Kernel::RegStage: {
      dim3 grid((unsigned)((p.N + BN - 1) / BN), (unsigned)((p.M + BM - 1) / BM)), block(THREADS);
      const size_t smem = 2 * 2 * TILE_BYTES;  // 73,728 B
      if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(gemm8_kernel<EPI>), smem, "hipFuncSetAttribute(gemm8_kernel)")) return rc;
      ao::launch(gemm8_kernel<EPI>, grid, block, smem, stream, p);
      AO_LAUNCH_CHECK("gemm8_kernel launch");
      return AO_OK;
    }
    default:
      set_error("gemm8: M=%d N=%d K=%d routed to no tiled kernel", p.M, p.N, p.K);
      return AO_ERR_INVALID_ARGUMENT;
  }
}

// the shapes the phase-interleaved 256 x 256 kernel takes from the two-stage tile kernels (product rule; see tiled_route)
bool gemm8_p8_band(int64_t M, int64_t N, int64_t K) {
  const int64_t big = ((N + 255) / 256) * ((M + 255) / 256), t128 = ((N + 127) / 128) * ((M + 127) / 128);
  return big >= 160 || (big >= 128 && (K <= 4096 || t128 > 512));
}

// The tiled GEMMs (every entry's last resort; the only path of the raw entries).  Variants: 1 the register-staged kernel; 2 / 4 / 8 / 16 the
// LDS-DMA kernel with 128 x 128 / 256 x 128 (4 waves: one wave per SIMD, measured 0.75-0.95x, nothing hides its ds_read -> MFMA latency) /
// 256 x 256 (8 waves) / 256 x 256 (4 waves of 128 x 128) tiles; 32 / 33 the phase-interleaved 256 x 256 / 256 x 128 kernels.
Gemm8Route tiled_route(int64_t M, int64_t N, int64_t K, bool aligned, const Gemm8Force& f) {
  if (K % BK != 0 || f.regstage) return Gemm8Route{Gemm8Kernel::RegStage, 128, 128};  // the LDS-DMA kernels need K % 128 == 0
  if (f.tile == 4) return Gemm8Route{Gemm8Kernel::Dma256x128, 256, 128};
  if (f.tile == 16) return Gemm8Route{Gemm8Kernel::Dma256x256w4, 256, 256};
  // (A 4-stage, 64-byte-K-step pipeline with hand-counted vmcnt was measured at 0.94-0.97x of these two-stage
  // kernels at both tile shapes, profiles/bench_8bit_r01_gemm.txt: the loop is LDS-read bound, not latency bound.)
  const int64_t big = ((N + 255) / 256) * ((M + 255) / 256);
  // The phase-interleaved 256 x 256 kernel (gemm8_p8_kernels.hip) once the problem has >= 160 such tiles.
  // Measured on the Llama-3-8B shapes (profiles/gemm8_variants_r02.txt, TOP/s int8, this kernel vs the two-stage kernels):
  // M = 8192: 2046 / 2084 / 2492 / 2796 vs 1557 / 1508 / 1777 / 2153; M = 2048: qkv (192 tiles) 1832 vs 1210, gate_up 2148 vs 1566,
  // but o / down (128 tiles: half the CUs idle) 1350 / 1710 vs 1330 / 1834; M = 512: gate_up (224 tiles) 2122 vs 1231.
  // Round 4 (profiles/gemm8_p8_band_r04.jsonl, cold weights): at 128 .. 159 such tiles it also wins while K <= 4096 (1024 x 8192 x 1024: 24.3 -> 20.2 us;
  // K = 8192 / 14336: 2 - 7 % behind) and whenever the 128 x 128 grid would need a second round of the chip (> 512 tiles: 1280 x 7168 x 8192 129 -> 84 us)
  if ((f.tile == 33 && gemm8_p8_fits(M, N, K)) || (f.tile == 0 && gemm8_p8h_band(M, N, K)))  // the 256 x 128 form
    return Gemm8Route{Gemm8Kernel::P8h, 256, 128, gemm8_p8h_parts(M, N, K, f.p8_split)};
  if ((f.tile == 32 || (f.tile == 0 && gemm8_p8_band(M, N, K))) && gemm8_p8_fits(M, N, K)) {
    // the persistent form (tuning key 6: 1 never, 2 wherever the shape allows) needs full tiles and aligned scales / output
    const bool full = M % 256 == 0 && N % 256 == 0 && K >= 256;
    const bool persistent = f.p8_persist != 1 && aligned && full && (f.p8_persist == 2 || gemm8_p8_persistent_shape(M, N, K));
    return Gemm8Route{persistent ? Gemm8Kernel::P8p : Gemm8Kernel::P8, 256, 256};
  }
  if (f.tile == 8 || (f.tile == 0 && big >= 512)) return Gemm8Route{Gemm8Kernel::Dma256, 256, 256};
  return Gemm8Route{Gemm8Kernel::Dma128, 128, 128};
}

int check_gemm_shape(const char* fn, int64_t M, int64_t N, int64_t K) {
  AO_REQUIRE(M >= 0 && N > 0 && K > 0, "%s: bad shape M=%lld N=%lld K=%lld", fn, (long long)M, (long long)N, (long long)K);
  AO_REQUIRE(K % 16 == 0, "%s: K=%lld must be a multiple of 16", fn, (long long)K);
  AO_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "%s: dimension too large", fn);
  AO_REQUIRE((M + BM - 1) / BM <= 65535, "%s: M=%lld too large for one launch", fn, (long long)M);
  return AO_OK;
}

bool aligned16(const void* row_scale, const void* col_scale, const void* bias, const void* out) {
  return (((uintptr_t)row_scale | (uintptr_t)col_scale | (uintptr_t)out) & 15) == 0 && ((uintptr_t)bias & 3) == 0;
}

thread_local Gemm8Force g_force;  // ao_gemm8_set_variant / ao_gemm8_set_tuning

}  // namespace

const Gemm8Force& gemm8_force() { return g_force; }

Gemm8Route gemm8_route(Gemm8Entry entry, int64_t M, int64_t N, int64_t K, bool aligned, const Gemm8Force& f) {
  const Gemm8Route invalid{};
  if (M <= 0 || N <= 0 || K <= 0 || K % 16 != 0) return invalid;
  Gemm8Route r;  // the per-tile streaming kernels: 16-wide n-tiles, K split among the waves of a workgroup
  switch (entry) {
    case Gemm8Entry::Int32Raw:
    case Gemm8Entry::Fp8Raw:
      return tiled_route(M, N, K, aligned, f);
    case Gemm8Entry::Int8Dyn:
    case Gemm8Entry::Fp8Dyn:
      // the fused form holds the cast activation in LDS: up to 16 rows of at most 64 KiB of codes (the decode kernel, else the round-3
      // GEMV), or 16 < M <= 256 through the mid-M kernel (two launches; K <= 16384)
      if (N % 16 != 0 || K % 128 != 0) return invalid;
      if (M <= 16) {
        if (M * (K + 16) > 64 * 1024) return invalid;
        r.kernel = dec8_plan(M, N, K, f.dec8, &r.dec) ? Gemm8Kernel::Dec8 : Gemm8Kernel::Dyn8;
        return r;
      }
      if (K > 16384 || !mid8_plan(M, N, K, f.mid8, &r.mid)) return invalid;
      r.kernel = Gemm8Kernel::Mid8;
      return r;
    case Gemm8Entry::Int8Scaled:
    case Gemm8Entry::Fp8Scaled:
      break;
  }
  const bool int8 = entry == Gemm8Entry::Int8Scaled;
  if (!int8 && N % 16 != 0) return invalid;
  // Weight-bandwidth-bound sizes stream the weights once instead of tiling a GEMM (Llama-70B TP8 shards, us per call,
  // profiles/bench_8bit_r01_fp8.jsonl):
  //   * M <= 16: the straight-line decode kernel; 16 < M <= 256, few output tiles, long K: the register-ring mid-M kernel (round 4);
  //   * M <= 32: stream8_kernels.hip -- activations straight from L2 per wave, no LDS staging, no split-K
  //     (gate_up 7168x8192: 15 us at M = 1, 20 at 16; the LDS-staged kernel below needs 23);
  //   * 32 < M and too few 128 x 128 tiles to fill the chip: rb8_kernels.hip (24 us at M = 64 where the kernel above
  //     needs 40; 27 us at M = 128 where the tiled GEMM needs 55); Llama-3-8B down_proj at M = 1 took 77 us through the tiled GEMM;
  //   * otherwise the tiled LDS-DMA GEMM.
  // Variants: 100 never a weight-streaming kernel; 101 / 102 always rb8 where the shape allows; an explicit tile variant never rb8.
  const bool rb_forced = f.rb >= 2, streaming = !rb_forced && !f.tiled_only, by_shape = !f.tiled_only && f.tile == 0 && !f.regstage;
  if (M <= 16 && streaming && dec8_plan(M, N, K, f.dec8, &r.dec)) {
    r.kernel = Gemm8Kernel::Dec8;
    return r;
  }
  if (M > 16 && streaming && by_shape && mid8_plan(M, N, K, f.mid8, &r.mid)) {
    r.kernel = Gemm8Kernel::Mid8;
    return r;
  }
  const bool rb_small = by_shape && rb8_small_m_preferred(M, N, K, f.rb);  // round 6
  bool rb;
  if (int8) {
    if (N % 16 == 0 && K % 128 == 0 && M <= 32 && !rb_small && streaming) r.kernel = Gemm8Kernel::Stream8;
    rb = N % 16 == 0 && (rb_small || rb8_preferred(M, N, K, f.rb));
  } else {
    // (at 32 < M <= 64 rb8 only wins once K is long enough to amortise its start-up and split-K meeting: o_proj shard 8192x1024 8.5 vs 10.9 us)
    // (round 4, cold weights -- every call of the replay reads another copy: the LDS-staged kernel wins from 33 rows on at every K of the
    // 70B / TP8 shards, down 8192 x 3584 at M = 64: 14.0 us against 20.9 through the per-tile kernel, o 8192 x 1024: 8.5 against 9.2; the
    // round-1 rule -- "only from K >= 4096 at 32 < M <= 64" -- had been measured on ONE re-used weight, i.e. out of the Infinity Cache)
    rb = rb_small || (rb8_preferred(M, N, K, f.rb) && (M > 32 || rb_forced));
    if (K % 128 == 0 && ((M <= 32 && !rb_small) || (M <= 64 && !rb)) && !(rb_forced && rb) && !f.tiled_only) r.kernel = Gemm8Kernel::Stream8;
  }
  if (r.kernel == Gemm8Kernel::Stream8) return r;
  if (rb) {
    r.kernel = Gemm8Kernel::Rb8;
    rb8_launch_plan(M, N, K, f, &r.tile_rows, &r.tile_cols, &r.k_parts);
    return r;
  }
  return tiled_route(M, N, K, aligned, f);
}

}  // namespace ao

using namespace ao;

extern "C" int ao_gemm8_set_variant(int variant) {
  Gemm8Force& f = g_force;
  f.regstage = variant == 1;
  f.tiled_only = variant == 100;
  f.tile = (variant == 2 || variant == 4 || variant == 8 || variant == 16 || variant == 32 || variant == 33) ? variant : 0;
  f.rb = variant == 101 ? 2 : variant == 102 ? 3 : (variant != 0 && variant < 110 && variant != 103) ? 1 : 0;
  f.rb8_1x8 = variant == 103;
  f.mx = (variant == 110) ? 1 : (variant == 111) ? 2 : 0;
  f.mx_stream = variant != 113;
  f.mx_quad = variant != 129;
  f.dec8 = (variant >= 200 && variant <= 299) ? variant : 0;
  f.mid8 = (variant >= 300 && variant <= 329) ? variant : 0;
  return AO_OK;
}

// 1 when the calling thread has any ao_gemm8_set_variant / ao_gemm8_set_tuning override set (tests assert the product dispatch)
extern "C" int ao_gemm8_overridden(void) {
  const Gemm8Force& f = g_force;
  const Gemm8Force d{};
  return !(f.regstage == d.regstage && f.tiled_only == d.tiled_only && f.tile == d.tile && f.rb == d.rb && f.rb8_1x8 == d.rb8_1x8 &&
           f.mx == d.mx && f.mx_stream == d.mx_stream && f.mx_quad == d.mx_quad && f.dec8 == d.dec8 && f.mid8 == d.mid8 &&
           f.rb8_bn == d.rb8_bn && f.rb8_split == d.rb8_split && f.rb8_bm == d.rb8_bm && f.p8_group_rows == d.p8_group_rows &&
           f.rb8_ablate == d.rb8_ablate && f.p8_persist == d.p8_persist && f.p8_split == d.p8_split && f.mx_proto == d.mx_proto);
}

extern "C" int ao_gemm8_set_tuning(int key, int value) {
  static int Gemm8Force::*const kKeys[] = {nullptr, &Gemm8Force::rb8_bn, &Gemm8Force::rb8_split, &Gemm8Force::rb8_bm, &Gemm8Force::p8_group_rows,
                                           &Gemm8Force::rb8_ablate, &Gemm8Force::p8_persist, &Gemm8Force::p8_split, nullptr,
                                           &Gemm8Force::mx_proto};
  AO_REQUIRE(key >= 1 && key <= 9, "ao_gemm8_set_tuning: unknown key %d", key);
  if (kKeys[key] != nullptr) g_force.*kKeys[key] = value;  // (key 8 selected gemm8_p8h's laboratory loop forms, which left the tree: accepted, ignored)
  return AO_OK;
}

namespace {

// the rowwise scaled entries: activation codes x weight codes, the scale epilogue, bf16 out
int gemm8_scaled(bool int8, const void* a, const float* scale_a, const void* b, const float* scale_b, const uint16_t* bias, uint16_t* y, int64_t M,
                 int64_t N, int64_t K, hipStream_t stream) {
  const Gemm8Route r = gemm8_route(int8 ? Gemm8Entry::Int8Scaled : Gemm8Entry::Fp8Scaled, M, N, K, aligned16(scale_a, scale_b, bias, y), g_force);
  switch (r.kernel) {
    case Gemm8Kernel::Dec8: return dec8_scaled(int8, a, scale_a, b, scale_b, bias, y, M, N, K, r.dec, stream);
    case Gemm8Kernel::Mid8: return mid8_scaled(int8, a, scale_a, b, scale_b, bias, y, M, N, K, r.mid, stream);
    case Gemm8Kernel::Rb8: return rb8_scaled(int8, a, b, scale_a, scale_b, bias, y, M, N, K, r.tile_rows, r.tile_cols, r.k_parts, stream);
    case Gemm8Kernel::Stream8:
      return int8 ? int8_scaled_stream(static_cast<const int8_t*>(a), static_cast<const int8_t*>(b), scale_a, scale_b, bias, y, M, N, K, stream)
                  : fp8_rowwise_stream(static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), scale_a, scale_b, bias, y, M, N, K, stream);
    default: break;
  }
  const Gemm8Args p{static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), scale_a, scale_b, bias, y, (int)M, (int)N, (int)K};
  return int8 ? launch_gemm8<EPI_INT8_SCALED>(r, p, stream) : launch_gemm8<EPI_FP8_ROWWISE>(r, p, stream);
}

const char* const kGemm8KernelNames[] = {"invalid", "dec8_kernel", "mid8_kernel", "stream8_kernel", "rb8_kernel", "gemm8_p8h_kernel",
                                         "gemm8_p8_kernel", "gemm8_p8p_kernel", "gemm8_dma_kernel<128x128>", "gemm8_dma_kernel<256x256>",
                                         "gemm8_dma_kernel<256x128>", "gemm8_dma_kernel<256x256,4 waves>", "gemm8_kernel", "dyn8_kernel"};
static_assert(sizeof(kGemm8KernelNames) / sizeof(kGemm8KernelNames[0]) == (size_t)Gemm8Kernel::Dyn8 + 1, "one name per Gemm8Kernel");

Gemm8Route product_route(int int8, int64_t M, int64_t N, int64_t K) {
  return gemm8_route(int8 ? Gemm8Entry::Int8Scaled : Gemm8Entry::Fp8Scaled, M, N, K, true, Gemm8Force{});
}

int gemm8_plan3(int int8, int64_t M, int64_t N, int64_t K, int* tile_rows, int* tile_cols, int* k_parts) {
  const Gemm8Route r = product_route(int8, M, N, K);
  AO_REQUIRE(r.kernel != Gemm8Kernel::Invalid, "ao_gemm8_plan: no kernel takes M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
  *tile_rows = r.tile_rows;
  *tile_cols = r.tile_cols;
  *k_parts = r.k_parts;
  return AO_OK;
}

}  // namespace

extern "C" int ao_int8_scaled_mm(const int8_t* xq, const float* x_scale, const int8_t* wq, const float* w_scale,
                                 const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K, void* stream) {
  if (int rc = check_gemm_shape(__func__, M, N, K)) return rc;
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(xq);
  AO_REQUIRE_PTR(x_scale);
  AO_REQUIRE_PTR(wq);
  AO_REQUIRE_PTR(w_scale);
  AO_REQUIRE_PTR(y);
  return gemm8_scaled(true, xq, x_scale, wq, w_scale, bias, y, M, N, K, (hipStream_t)stream);
}

// Which kernel ao_fp8_scaled_mm / ao_int8_scaled_mm launch for a shape with 16-byte-aligned operands and no override set (host logic
// only: no launch, no GPU).  tests/test_host_dispatch.py pins the table.
extern "C" const char* ao_gemm8_kernel_name(int int8, int64_t M, int64_t N, int64_t K) {
  return kGemm8KernelNames[(int)product_route(int8, M, N, K).kernel];
}

// The launch shape of that route: tile rows, column-tile width and K parts (host logic only).
extern "C" int ao_gemm8_plan(int int8, int64_t M, int64_t N, int64_t K, int* tile_cols, int* k_parts) {
  AO_REQUIRE_PTR(tile_cols);
  AO_REQUIRE_PTR(k_parts);
  int rows = 0;
  return gemm8_plan3(int8, M, N, K, &rows, tile_cols, k_parts);
}
extern "C" int ao_gemm8_plan_rows(int int8, int64_t M, int64_t N, int64_t K, int* tile_rows) {
  AO_REQUIRE_PTR(tile_rows);
  int cols = 0, parts = 0;
  return gemm8_plan3(int8, M, N, K, tile_rows, &cols, &parts);
}

// Every field of the product route of one entry point (host logic only): tests derive their case list from it.
extern "C" int ao_gemm8_route(int entry, int64_t M, int64_t N, int64_t K, int aligned, int32_t* out, int cap) {
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(entry >= 0 && entry <= (int)Gemm8Entry::Fp8Dyn, "ao_gemm8_route: unknown entry %d", entry);
  AO_REQUIRE(cap >= 11, "ao_gemm8_route: out holds %d fields, the route has 11", cap);
  const Gemm8Route r = gemm8_route((Gemm8Entry)entry, M, N, K, aligned != 0, Gemm8Force{});
  const int32_t v[11] = {(int32_t)r.kernel, r.tile_rows, r.tile_cols, r.k_parts, r.dec.waves, r.dec.depth,
                         r.dec.loop, r.dec.half, r.dec.rows8, r.mid.mt, r.mid.split};
  for (int i = 0; i < 11; ++i) out[i] = v[i];
  return AO_OK;
}

extern "C" int ao_int8_int_mm(const int8_t* a, const int8_t* b_t, int32_t* c, int64_t M, int64_t N, int64_t K,
                              void* stream) {
  if (int rc = check_gemm_shape(__func__, M, N, K)) return rc;
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(a);
  AO_REQUIRE_PTR(b_t);
  AO_REQUIRE_PTR(c);
  const Gemm8Route r = gemm8_route(Gemm8Entry::Int32Raw, M, N, K, aligned16(nullptr, nullptr, nullptr, c), g_force);
  Gemm8Args p{reinterpret_cast<const uint8_t*>(a), reinterpret_cast<const uint8_t*>(b_t), nullptr, nullptr, nullptr, c,
              (int)M, (int)N, (int)K};
  return launch_gemm8<EPI_INT32>(r, p, (hipStream_t)stream);
}

// Unscaled e4m3 x e4m3 products, fp32 out: the partial sums a K-sharded (row-parallel) fp8 linear all-reduces before
// ao_fp8_scale_epilogue applies scale_a[m] * scale_b[n] (+ bias) once, like the unsharded aten::_scaled_mm.
extern "C" int ao_fp8_mm_f32(const uint8_t* a, const uint8_t* b, float* c, int64_t M, int64_t N, int64_t K, void* stream) {
  if (int rc = check_gemm_shape(__func__, M, N, K)) return rc;
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(a);
  AO_REQUIRE_PTR(b);
  AO_REQUIRE_PTR(c);
  const Gemm8Route r = gemm8_route(Gemm8Entry::Fp8Raw, M, N, K, aligned16(nullptr, nullptr, nullptr, c), g_force);
  Gemm8Args p{a, b, nullptr, nullptr, nullptr, c, (int)M, (int)N, (int)K};
  return launch_gemm8<EPI_FP8_RAW>(r, p, (hipStream_t)stream);
}

extern "C" int ao_fp8_scaled_mm(const uint8_t* a, const uint8_t* b, const float* scale_a, const float* scale_b,
                                const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K, void* stream) {
  if (int rc = check_gemm_shape(__func__, M, N, K)) return rc;
  AO_REQUIRE(N % 16 == 0, "ao_fp8_scaled_mm: N=%lld must be a multiple of 16", (long long)N);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(a);
  AO_REQUIRE_PTR(b);
  AO_REQUIRE_PTR(scale_a);
  AO_REQUIRE_PTR(scale_b);
  AO_REQUIRE_PTR(y);
  return gemm8_scaled(false, a, scale_a, b, scale_b, bias, y, M, N, K, (hipStream_t)stream);
}
