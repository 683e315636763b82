// The 128 x 128 tile walk of the NVFP4 training casts (nvfp4_train_kernels.hip: the dense entries; nvfp4_grouped_train_kernels.hip: the
// MoE grouped entries), nvfp4_train_cast_kernel<W2D, SR, GROUPED>: a workgroup of 256 threads owns a 128 x 128 tile of the bf16 source.
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
// GROUPED changes what a tile is cast UNDER, nothing of the walk:
//   W2D      the source is [E][M][N]; blockIdx.z is the expert, every pointer moves by the expert's stride in 64 bits and the amax is
//            amax[e]: expert e is the dense cast of w[e], byte for byte.
//   not W2D  the source's rows are token groups (offs[E], cumulative ends, multiples of 16); the tile's eight 16-row runs look up their
//            group once (the first e with offs[e] > the run's first row) and park its two encode scales in LDS; a run is cast under
//            amax[e][0] (column output) and amax[e][1] (row output).  A run at or past offs[E-1] -- a capacity row -- is written as zero
//            codes and zero scale bytes in both outputs.  The stochastic-rounding counter is the dense one: the dword's index in the WHOLE
//            output, so one group of every row, or equal amax pairs, give the dense bytes.  offs is only ever compared with row numbers:
//            whatever it holds, every address comes from the tile.
#pragma once
#include "common.h"
#include "quant_math.h"

namespace ao {
namespace nvfp4_train {

constexpr int kT = 128;                    // tile rows and columns
constexpr int kThreads = 256;
constexpr int kInStride = 2 * kT + 16;     // bytes between two rows of the staged bf16 tile (16-byte aligned row blocks)
constexpr int kOutStride = kT / 2 + 8;     // bytes between two columns of the staged transposed codes
constexpr int kUnits = kT * (kT / 16) / kThreads;  // blocks of 16 a thread casts per direction

struct TrainCastArgs {
  const uint16_t* x;        // bf16 [M][N] (grouped W2D: [E][M][N])
  const float* amax_col;    // the per-tensor amax of the column output's values (grouped: [e][0] of [E][2]; grouped W2D: [E])
  const float* amax_row;    // the per-tensor amax of the row output's values (grouped: [e][1]; grouped W2D: [E])
  uint32_t sign_mask;       // bit i set: s_i = -1
  const int64_t* sr_seed;   // SR only
  const int64_t* col_offset;
  const int64_t* row_offset;
  uint8_t* col_q;           // [N][M/2] or null
  uint8_t* col_s;           // [N][M/16]
  uint8_t* row_q;           // [M][N/2] or null
  uint8_t* row_s;           // [M][N/16]
  int64_t M, N;
  const int32_t* offs;      // grouped, not W2D: [E] cumulative group ends along M
  int E;
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

// The group of a row: the first e with offs[e] > row, E when there is none (a capacity row).  A binary search that ends for any contents.
__device__ __forceinline__ int group_of_row(const int32_t* offs, int E, int64_t row) {
  int lo = 0, hi = E;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)offs[mid] > row) hi = mid; else lo = mid + 1;
  }
  return lo;
}

template <bool W2D, bool SR, bool GROUPED>
__global__ __launch_bounds__(kThreads) void nvfp4_train_cast_kernel(TrainCastArgs p) {
  __shared__ __attribute__((aligned(16))) uint8_t tin[kT * kInStride];
  __shared__ __attribute__((aligned(16))) uint8_t tout[kT * kOutStride];
  __shared__ uint8_t tsc[kT * 8];
  __shared__ float bam[W2D ? kT : 1][8];
  constexpr bool kRuns = GROUPED && !W2D;  // the tile's 16-row runs are cast under their groups' amaxes
  // (sized 1 and never touched where kRuns is false: those instances keep the LDS they had)
  __shared__ Nvfp4TrainGlobal run_gl[kRuns ? 2 : 1][kRuns ? kT / 16 : 1];  // [0]: column output, [1]: row output
  __shared__ int run_ok[kRuns ? kT / 16 : 1];                               // 0: a capacity run
  const int tid = threadIdx.x;
  const int64_t m0 = (int64_t)blockIdx.y * kT, n0 = (int64_t)blockIdx.x * kT;
  if constexpr (GROUPED && W2D) {
    const size_t e = blockIdx.z, mn = (size_t)p.M * (size_t)p.N;
    p.x += e * mn;
    p.amax_col += e;
    p.amax_row += e;
    p.col_q += e * (mn >> 1);
    p.col_s += e * (mn >> 4);
    p.row_q += e * (mn >> 1);
    p.row_s += e * (mn >> 4);
  }
  const bool do_row = p.row_q != nullptr, do_col = p.col_q != nullptr;
  uint32_t k0 = 0u, k1 = 0u, row_off = 0u, col_off = 0u;
  if (SR) {
    const uint64_t seed = (uint64_t)*p.sr_seed;
    k0 = (uint32_t)seed;
    k1 = (uint32_t)(seed >> 32);
    if (do_row) row_off = (uint32_t)(uint64_t)*p.row_offset;
    if (do_col) col_off = (uint32_t)(uint64_t)*p.col_offset;
  }
  if constexpr (kRuns) {
    if (tid < kT / 16) {
      const int64_t row = m0 + 16 * tid;
      const int g = row < p.M ? group_of_row(p.offs, p.E, row) : p.E;
      run_ok[tid] = g < p.E;
      if (g < p.E) {
        run_gl[0][tid] = nvfp4_train_global(p.amax_col[2 * g]);
        run_gl[1][tid] = nvfp4_train_global(p.amax_row[2 * g]);
      }
    }
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
  if (W2D || kRuns || do_col) __syncthreads();
  // 2. the row output, from the registers
  if (do_row) {
    Nvfp4TrainGlobal gl = {};
    if constexpr (!kRuns) gl = nvfp4_train_global(*p.amax_row);
#pragma unroll
    for (int u = 0; u < kUnits; ++u) {
      const int id = u * kThreads + tid, r = id >> 3, cb = id & 7;
      const int64_t gm = m0 + r, gn = n0 + 16 * cb;
      if (gm < p.M && gn < p.N) {
        u32x2 q = {0u, 0u};
        uint32_t s8 = 0u;
        bool cast = true;
        if constexpr (kRuns) {
          cast = run_ok[r >> 4] != 0;
          gl = run_gl[1][r >> 4];
        }
        if (cast) {
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
          const float enc = nvfp4_train_encode(bm, gl, s8);
          q = nvfp4_train_codes16<SR>(a, enc, (uint64_t)(gm * p.N + gn) >> 3, row_off, 0u, k0, k1);
        }
        *reinterpret_cast<u32x2*>(p.row_q + gm * (p.N >> 1) + (gn >> 1)) = q;
        p.row_s[gm * (p.N >> 4) + (gn >> 4)] = (uint8_t)s8;
      }
    }
  }
  if (!do_col) return;  // (workgroup-uniform)
  // 3. the column output: 16 rows of one column a thread, staged transposed
  Nvfp4TrainGlobal gl = {};
  if constexpr (!kRuns) gl = nvfp4_train_global(*p.amax_col);
#pragma unroll
  for (int u = 0; u < kUnits; ++u) {
    const int id = u * kThreads + tid, c = id & (kT - 1), mb = id >> 7;
    const int64_t gn = n0 + c, gm = m0 + 16 * mb;
    if (gn < p.N && gm < p.M) {  // (16 | M)
      u32x2 q = {0u, 0u};
      uint32_t s8 = 0u;
      bool cast = true;
      if constexpr (kRuns) {
        cast = run_ok[mb] != 0;
        gl = run_gl[0][mb];
      }
      if (cast) {
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
        const float enc = nvfp4_train_encode(bm, gl, s8);
        q = nvfp4_train_codes16<SR>(a, enc, (uint64_t)(gn * p.M + gm) >> 3, col_off, 1u, k0, k1);
      }
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

inline int check_mn(const char* fn, int64_t M, int64_t N) {
  AO_REQUIRE(M >= 0 && N > 0 && M % 16 == 0 && N % 16 == 0 && M < (1ll << 31) && N < (1ll << 31) && M * N < (1ll << 40),
             "%s: bad shape %lld x %lld (both multiples of 16, columns > 0, each below 2^31 and the product below 2^40)", fn, (long long)M,
             (long long)N);
  return AO_OK;
}

// the instances that have a caller: the activation cast under either rounding, the weight cast under round to nearest even; experts: the
// grid's z extent (1: dense)
template <bool W2D, bool SR, bool GROUPED>
int launch_cast(const TrainCastArgs& a, int64_t experts, hipStream_t st) {
  static_assert(!(W2D && SR), "the weight is never rounded stochastically");
  const dim3 grid((unsigned)((a.N + kT - 1) / kT), (unsigned)((a.M + kT - 1) / kT), (unsigned)experts);
  ao::launch(nvfp4_train_cast_kernel<W2D, SR, GROUPED>, grid, dim3(kThreads), 0, st, a);
  AO_LAUNCH_CHECK("nvfp4_train_cast_kernel launch");
  return AO_OK;
}

}  // namespace nvfp4_train
}  // namespace ao
