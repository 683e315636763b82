// Int8 mixed-precision training (torchao/prototype/quantized_training/int8.py, int8_mixed_precision.py, int8_mm.py) on gfx950: the absmax
// casts of a linear's three GEMMs and a scaled int8 GEMM that takes either operand in either layout.  The arithmetic, every step ONE fp32
// operation rounded once, the divisions IEEE:
//   cast   scale = bf16(amax / 127);  inv = 1 / max(f32(scale), eps);  v = f32(x) * inv;  q = clip(rint(v), -128, 127), rint to even;
//          under stochastic rounding q = clip(floor(v + u), -128, 127), u = (w >> 8) 2^-24 with w word (e & 3) of
//          philox4x32_10(counter (e >> 2, offset), key seed), e the element's index in the tensor (this library's contract)
//   mm     y = bf16((f32(acc) * f32(sa[m])) * f32(sb[n])), acc = sum_c A[m, c] B[n, c] in int32: exact, so any order of c gives the same bits
// No cast writes a transposed matrix.  A row cast has one scale a row, a column cast one a column (the amax taken down dim 0), and both leave
// the code of x[r][c] at [r][c].  The column amax needs the whole column before the first code, so a cast with columns is two reads of x:
//   amax   grid (strips of 32 rows, chunks of 4096 columns); a wave walks whole rows of its chunk, a lane keeps the running |x| of its 64
//          columns as packed 16-bit maxima (|bf16| bits order as integers: one v_and + one v_pk_max_u16 a dword) and the row's maximum
//          beside them.  A workgroup leaves one 16-bit maximum a column and one a row: partials, no atomics, the same bits every run
//   scale  the column partials of all strips -> s_col
//   cast   grid (blocks of 32 rows, blocks of 1024 columns); a lane owns 16 columns -- its 16 reciprocals stay in registers down the rows,
//          and a row of codes is one 16-byte store a lane for either direction
// Rows alone are one launch and one read: a workgroup holds its row in registers (up to 16384 columns) between the amax and the codes.
//
// The GEMM: 128 x 128 output tile, contraction steps of 64, three LDS stages filled by global_load_lds in 16-byte pieces along whichever
// dimension of the operand is contiguous; four waves as 2 x 2, a wave owns 64 x 64 = 4 x 4 tiles of v_mfma_i32_16x16x64_i8.
//   flag 0 (contraction innermost)   stage = [128 rows][64 bytes], piece c of row r in slot c ^ ((r >> 2) & 3); a lane's MFMA operand is the
//                                    16 contiguous bytes k = 16 kq .. 16 kq + 15 of its row: one ds_read_b128
//   flag 1 (contraction outermost)   stage = [64 k][128 rows], the 16-row piece p of k row k in slot p ^ (k & 7); the operand comes out of two
//                                    ds_read_b64_tr_b8.  Measured on the MI355X: in a group of 16 lanes, byte b of lane i is byte (i & 7) of the
//                                    8 bytes lane 2 b + (i >> 3) addressed.  Lane s addresses rows 8 (s & 1) .. + 7 of k row k0 + (s >> 1):
//                                    lane i then holds row i at k0 .. k0 + 7 in order -- two loads give k = 16 kq .. 16 kq + 15, the very
//                                    order of flag 0, so the two kinds meet in one MFMA without a shuffle
// Rows past an edge read a valid row (never stored).  The contraction's ragged last step is zero-filled: a piece past Kc is not requested,
// its lane writes 16 zero bytes in its place.
#include "common.h"
#include "lds_dma.h"
#include "quant_math.h"

#include <algorithm>

namespace ao {
namespace {

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

constexpr int kStripRows = 32;    // rows of an amax / cast workgroup: 8 a wave
constexpr int kAmaxChunk = 4096;  // columns of an amax workgroup: 8 vectors of 8 a lane
constexpr int kCastCols = 1024;   // columns of a cast workgroup: 16 a lane

struct SrKey {
  int on;
  uint32_t seed_lo, seed_hi, off_lo, off_hi;
};

__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
// the running packed |x| maxima of the four dwords of a vector; returns the vector's own maximum pair
__device__ __forceinline__ uint32_t abs_max4(const u32x4& v, uint32_t (&m)[4]) {
  const uint32_t a0 = v.x & 0x7fff7fffu, a1 = v.y & 0x7fff7fffu, a2 = v.z & 0x7fff7fffu, a3 = v.w & 0x7fff7fffu;
  m[0] = pk_max_u16(m[0], a0), m[1] = pk_max_u16(m[1], a1), m[2] = pk_max_u16(m[2], a2), m[3] = pk_max_u16(m[3], a3);
  return pk_max_u16(pk_max_u16(a0, a1), pk_max_u16(a2, a3));
}
__device__ __forceinline__ uint32_t abs_max4(const u32x4& v) {
  return pk_max_u16(pk_max_u16(v.x & 0x7fff7fffu, v.y & 0x7fff7fffu), pk_max_u16(v.z & 0x7fff7fffu, v.w & 0x7fff7fffu));
}
__device__ __forceinline__ float pair_max_f32(uint32_t pk) { return bf16_lo_to_f32(max(pk & 0xffffu, pk >> 16)); }

__device__ __forceinline__ float train_scale(float amax) { return round_bf16(amax / 127.0f); }
__device__ __forceinline__ float train_inv(float scale, float eps) { return 1.0f / fmaxf(scale, eps); }

__device__ __forceinline__ uint32_t code_rn(float x, float inv) { return (uint32_t)(int)fminf(fmaxf(rintf(x * inv), -128.f), 127.f) & 0xffu; }
__device__ __forceinline__ uint32_t code_sr(float x, float inv, uint32_t w) {
#pragma clang fp contract(off)
  const float v = x * inv;
  const float u = (float)(w >> 8) * 0x1p-24f;
  return (uint32_t)(int)fminf(fmaxf(floorf(v + u), -128.f), 127.f) & 0xffu;
}

// the row codes of 16 adjacent elements, e0 the index of the first in the tensor
__device__ __forceinline__ u32x4 row_codes16(const u32x4& v0, const u32x4& v1, float inv, const SrKey& sr, uint64_t e0) {
  if (!sr.on) {
    const u32x2 a = int8_quant8(v0, inv), b = int8_quant8(v1, inv);
    return u32x4{a.x, a.y, b.x, b.y};
  }
  float f[16];
  unpack_bf16x8(v0, *reinterpret_cast<float(*)[8]>(f));
  unpack_bf16x8(v1, *reinterpret_cast<float(*)[8]>(f + 8));
  uint32_t out[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const uint64_t c = (e0 >> 2) + g;
    const Philox4 r = philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), sr.off_lo, sr.off_hi, sr.seed_lo, sr.seed_hi);
    out[g] = code_sr(f[4 * g], inv, r.w[0]) | (code_sr(f[4 * g + 1], inv, r.w[1]) << 8) | (code_sr(f[4 * g + 2], inv, r.w[2]) << 16) |
             (code_sr(f[4 * g + 3], inv, r.w[3]) << 24);
  }
  return u32x4{out[0], out[1], out[2], out[3]};
}

// ---- rows alone: one workgroup a row, NP 16-column pieces a thread kept in registers (0: the row is read a second time, from cache) ------------
template <int NP>
__global__ __launch_bounds__(kRowThreads) void int8_train_rows_kernel(const uint16_t* x, int8_t* q, uint16_t* scale, int C, float eps, SrKey sr) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const u32x4* xr = reinterpret_cast<const u32x4*>(x + row * C);
  u32x4* qr = reinterpret_cast<u32x4*>(q + row * C);
  const int pieces = C >> 4;
  constexpr int kHeld = NP > 0 ? NP : 1;
  u32x4 v[kHeld][2];
  uint32_t m = 0u;
  if (NP > 0) {
#pragma unroll
    for (int j = 0; j < kHeld; ++j) {
      const int pc = threadIdx.x + j * kRowThreads;
      v[j][0] = v[j][1] = u32x4{0u, 0u, 0u, 0u};
      if (pc < pieces) v[j][0] = __builtin_nontemporal_load(xr + 2 * pc), v[j][1] = __builtin_nontemporal_load(xr + 2 * pc + 1);
      m = pk_max_u16(m, pk_max_u16(abs_max4(v[j][0]), abs_max4(v[j][1])));
    }
  } else {
    for (int pc = threadIdx.x; pc < pieces; pc += kRowThreads) m = pk_max_u16(m, pk_max_u16(abs_max4(xr[2 * pc]), abs_max4(xr[2 * pc + 1])));
  }
  const float s = train_scale(block_max(pair_max_f32(m), red));
  const float inv = train_inv(s, eps);
  if (NP > 0) {
#pragma unroll
    for (int j = 0; j < kHeld; ++j) {
      const int pc = threadIdx.x + j * kRowThreads;
      if (pc < pieces) qr[pc] = row_codes16(v[j][0], v[j][1], inv, sr, (uint64_t)row * C + ((uint64_t)pc << 4));
    }
  } else {
    for (int pc = threadIdx.x; pc < pieces; pc += kRowThreads)
      qr[pc] = row_codes16(xr[2 * pc], xr[2 * pc + 1], inv, sr, (uint64_t)row * C + ((uint64_t)pc << 4));
  }
  if (threadIdx.x == 0) scale[row] = f32_to_bf16_bits(s);
}

// ---- with columns, pass 1: the partial maxima.  grid (strips, chunks).  colpart [strips][C], rowpart [R][chunks] (null: no row cast) ------------
__global__ __launch_bounds__(256) void int8_train_amax_kernel(const uint16_t* x, uint16_t* colpart, uint16_t* rowpart, int R, int C) {
  __shared__ uint32_t cm[4][kAmaxChunk / 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = blockIdx.y * kAmaxChunk, r0 = blockIdx.x * kStripRows;
  uint32_t colm[8][4];
#pragma unroll
  for (int j = 0; j < 8; ++j) colm[j][0] = colm[j][1] = colm[j][2] = colm[j][3] = 0u;
  for (int i = 0; i < kStripRows / 4; ++i) {
    const int r = r0 + wave + 4 * i;
    if (r >= R) break;
    const uint16_t* xr = x + (int64_t)r * C;
    uint32_t rm = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = c0 + ((lane + 64 * j) << 3);
      if (col < C) rm = pk_max_u16(rm, abs_max4(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(xr + col)), colm[j]));
    }
    if (rowpart != nullptr) {
      const float f = wave_max(pair_max_f32(rm));
      if (lane == 0) rowpart[(int64_t)r * gridDim.y + blockIdx.y] = (uint16_t)(f32_to_bits(f) >> 16);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int d = 0; d < 4; ++d) cm[wave][((lane + 64 * j) << 2) + d] = colm[j][d];
  __syncthreads();
  for (int i = threadIdx.x; i < kAmaxChunk / 2; i += 256) {
    const int col = c0 + 2 * i;
    if (col < C)
      *reinterpret_cast<uint32_t*>(colpart + (int64_t)blockIdx.x * C + col) = pk_max_u16(pk_max_u16(cm[0][i], cm[1][i]), pk_max_u16(cm[2][i], cm[3][i]));
  }
}

// pass 1b: the strips' partials -> the column scales, two columns a thread
__global__ __launch_bounds__(256) void int8_train_col_scale_kernel(const uint16_t* colpart, int strips, int C, uint16_t* s_col) {
  const int col = (blockIdx.x * 256 + threadIdx.x) * 2;
  if (col >= C) return;
  uint32_t m = 0u;
  for (int s = 0; s < strips; ++s) m = pk_max_u16(m, *reinterpret_cast<const uint32_t*>(colpart + (int64_t)s * C + col));
  *reinterpret_cast<uint32_t*>(s_col + col) =
      (uint32_t)f32_to_bf16_bits(train_scale(bf16_lo_to_f32(m & 0xffffu))) | ((uint32_t)f32_to_bf16_bits(train_scale(bf16_lo_to_f32(m >> 16))) << 16);
}

// pass 2: the codes of both directions from one read.  grid (blocks of 32 rows, blocks of 1024 columns)
__global__ __launch_bounds__(256) void int8_train_cast_kernel(const uint16_t* x, const uint16_t* s_col, const uint16_t* rowpart, int chunks, int8_t* q_row,
                                                              uint16_t* s_row, int8_t* q_col, int R, int C, float eps, SrKey sr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.y * kCastCols + (lane << 4);
  if (col >= C) return;
  float invc[16];
  {
    const u32x4 s0 = *reinterpret_cast<const u32x4*>(s_col + col), s1 = *reinterpret_cast<const u32x4*>(s_col + col + 8);
    unpack_bf16x8(s0, *reinterpret_cast<float(*)[8]>(invc));
    unpack_bf16x8(s1, *reinterpret_cast<float(*)[8]>(invc + 8));
#pragma unroll
    for (int j = 0; j < 16; ++j) invc[j] = train_inv(invc[j], eps);
  }
  for (int i = 0; i < kStripRows / 4; ++i) {
    const int r = blockIdx.x * kStripRows + wave + 4 * i;
    if (r >= R) break;
    const int64_t e0 = (int64_t)r * C + col;
    const u32x4 v0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(x + e0));
    const u32x4 v1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(x + e0 + 8));
    if (q_row != nullptr) {
      uint32_t m = 0u;
      for (int c = 0; c < chunks; ++c) m = max(m, (uint32_t)rowpart[(int64_t)r * chunks + c]);
      const float s = train_scale(bf16_lo_to_f32(m));
      *reinterpret_cast<u32x4*>(q_row + e0) = row_codes16(v0, v1, train_inv(s, eps), sr, (uint64_t)e0);
      if (blockIdx.y == 0 && lane == 0) s_row[r] = f32_to_bf16_bits(s);
    }
    float f[16];
    unpack_bf16x8(v0, *reinterpret_cast<float(*)[8]>(f));
    unpack_bf16x8(v1, *reinterpret_cast<float(*)[8]>(f + 8));
    uint32_t o[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      o[g] = code_rn(f[4 * g], invc[4 * g]) | (code_rn(f[4 * g + 1], invc[4 * g + 1]) << 8) | (code_rn(f[4 * g + 2], invc[4 * g + 2]) << 16) |
             (code_rn(f[4 * g + 3], invc[4 * g + 3]) << 24);
    *reinterpret_cast<u32x4*>(q_col + e0) = u32x4{o[0], o[1], o[2], o[3]};
  }
}

// ---- the GEMM ---------------------------------------------------------------------------------------------------------------------------------
struct TrainMmArgs {
  const int8_t* a;     // flag 0: [M][Kc], flag 1: [Kc][M]
  const int8_t* b;     // flag 0: [N][Kc], flag 1: [Kc][N]
  const uint16_t* sa;  // [M] bf16
  const uint16_t* sb;  // [N] bf16
  uint16_t* out;       // [M][N] bf16
  int M, N, Kc;
};

constexpr int kMmTile = 128, kMmK = 64, kMmStages = 3;
constexpr int kMmOpBytes = kMmTile * kMmK;  // one operand of one stage: 8 KiB either way round
constexpr int kMmDmaPerStep = 4;            // DMA instructions a wave issues a step: two an operand

// One operand of the tile: where this lane's two DMA pieces of a step come from, and how the MFMA operand is read back.
template <bool T>
struct TrainOperand {
  const char* base;  // the tile's first byte at step 0
  int64_t step;      // bytes from one step's base to the next
  uint32_t v[2];     // this lane's source offsets from the step base
  int k[2];          // the contraction index inside the step at which piece i starts (its k row under flag 1)

  // rows0: the tile's first row, rows: the operand's rows, ld: its contiguous dimension (Kc under flag 0, rows under flag 1)
  __device__ __forceinline__ void init(const int8_t* p, int rows0, int rows, int Kc, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (!T) {
        const int r = min(32 * wave + 16 * i + (lane >> 2), rows - 1 - rows0);
        k[i] = ((lane & 3) ^ (lane >> 4)) << 4;
        v[i] = (uint32_t)r * (uint32_t)Kc + (uint32_t)k[i];
      } else {
        k[i] = 16 * wave + 8 * i + (lane >> 3);
        v[i] = (uint32_t)k[i] * (uint32_t)rows + (uint32_t)min(((lane & 7) ^ (lane >> 3)) << 4, rows - 16 - rows0);
      }
    }
    base = reinterpret_cast<const char*>(p) + (T ? (int64_t)rows0 : (int64_t)rows0 * Kc);
    step = T ? (int64_t)kMmK * rows : (int64_t)kMmK;
  }
  __device__ __forceinline__ void issue(int t, uint32_t lds_dst) const { dma_b128_x2(base + t * step, v[0], v[1], lds_dst); }
  // the ragged last step: a piece at or past Kc is zero bytes (stage: this wave's 2 KiB of the buffer, as a pointer)
  __device__ __forceinline__ void issue_tail(int t, int Kc, uint32_t lds_dst, char* stage, int lane) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (t * kMmK + k[i] < Kc) dma_b128_s(base + t * step, v[i], lds_dst + i * 1024);
      else *reinterpret_cast<u32x4*>(stage + i * 1024 + lane * 16) = u32x4{0u, 0u, 0u, 0u};
    }
  }
  // the MFMA operand of lane (ml, kq) for the 16 rows at r0 (a multiple of 16) of the staged tile: k = 16 kq .. 16 kq + 15 in order
  static __device__ __forceinline__ i32x4 frag(const char* buf, int r0, int ml, int kq) {
    if (!T) return *reinterpret_cast<const i32x4*>(buf + (r0 + ml) * kMmK + ((kq ^ ((ml >> 2) & 3)) << 4));
    typedef __attribute__((address_space(3))) i32x2* lds_i32x2;
    const int kr = ml >> 1;  // the k row inside a group of 8, which is also its swizzle key
    const char* p = buf + (16 * kq + kr) * kMmTile + (((r0 >> 4) ^ kr) << 4) + ((ml & 1) << 3);
    const i32x2 lo = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2)(p));
    const i32x2 hi = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2)(p + 8 * kMmTile));
    return i32x4{lo.x, lo.y, hi.x, hi.y};
  }
};

__device__ __forceinline__ uint32_t train_out2(int a0, int a1, float sa, float sb0, float sb1) {
#pragma clang fp contract(off)
  return pack_bf16x2(((float)a0 * sa) * sb0, ((float)a1 * sa) * sb1);
}

template <bool AT, bool BT>
__global__ __launch_bounds__(256) void int8_train_mm_kernel(TrainMmArgs p) {
  __shared__ __attribute__((aligned(16))) char As[kMmStages][kMmOpBytes];
  __shared__ __attribute__((aligned(16))) char Bs[kMmStages][kMmOpBytes];
  const int tid = threadIdx.x, lane = tid & 63, ml = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * kMmTile, n0 = blockIdx.x * kMmTile;
  const int T = (p.Kc + kMmK - 1) / kMmK;
  const bool ragged = (p.Kc % kMmK) != 0;

  TrainOperand<AT> A;
  TrainOperand<BT> B;
  A.init(p.a, m0, p.M, p.Kc, wave, lane);
  B.init(p.b, n0, p.N, p.Kc, wave, lane);
  auto issue = [&](int t) {
    const int buf = t % kMmStages;
    if (ragged && t == T - 1) {
      A.issue_tail(t, p.Kc, lds_offset(As[buf]) + wave * 2048, As[buf] + wave * 2048, lane);
      B.issue_tail(t, p.Kc, lds_offset(Bs[buf]) + wave * 2048, Bs[buf] + wave * 2048, lane);
    } else {
      A.issue(t, lds_offset(As[buf]) + wave * 2048);
      B.issue(t, lds_offset(Bs[buf]) + wave * 2048);
    }
  };

  i32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

  issue(0);
  if (T > 1) issue(1);
  for (int t = 0; t < T; ++t) {
    // step t has landed for this wave (the DMAs return in order; the last step may hold fewer than kMmDmaPerStep, so nothing is left in
    // flight behind the last two); past the barrier for every wave, and stage (t + 2) % 3 = (t - 1) % 3 has been read out
    if (t + 2 < T) wait_vmcnt<kMmDmaPerStep>();
    else wait_vmcnt<0>();
    lds_barrier();
    if (t + 2 < T) issue(t + 2);
    const char* Ab = As[t % kMmStages];
    const char* Bb = Bs[t % kMmStages];
    i32x4 bop[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bop[j] = TrainOperand<BT>::frag(Bb, wn * 64 + j * 16, ml, kq);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const i32x4 aop = TrainOperand<AT>::frag(Ab, wm * 64 + i * 16, ml, kq);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bop[j], aop, acc[i][j], 0, 0, 0);
    }
  }

  // B was the MFMA's first operand: lane (row ml of the m-tile, group kq) holds columns 4 kq .. + 3 of the n-tile
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + ml;
    if (m >= p.M) continue;
    const float rs = bf16_lo_to_f32(p.sa[m]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + kq * 4;
      if (n >= p.N) continue;  // (N % 16 == 0: the four columns stand or fall together)
      const u32x2 cs = *reinterpret_cast<const u32x2*>(p.sb + n);
      *reinterpret_cast<u32x2*>(p.out + (size_t)m * p.N + n) =
          u32x2{train_out2(acc[i][j][0], acc[i][j][1], rs, bf16_lo_to_f32(cs.x), bf16_hi_to_f32(cs.x)),
                train_out2(acc[i][j][2], acc[i][j][3], rs, bf16_lo_to_f32(cs.y), bf16_hi_to_f32(cs.y))};
    }
  }
}

int train_mm_check_shape(const char* fn, int64_t M, int64_t N, int64_t Kc, int a_t, int b_t) {
  AO_REQUIRE((a_t == 0 || a_t == 1) && (b_t == 0 || b_t == 1), "%s: a_t=%d and b_t=%d must be 0 (contraction innermost) or 1 (outermost)", fn, a_t, b_t);
  AO_REQUIRE(M >= 0 && N >= 0 && Kc >= 1, "%s: bad shape M=%lld N=%lld Kc=%lld", fn, (long long)M, (long long)N, (long long)Kc);
  AO_REQUIRE(N % 16 == 0, "%s: N=%lld must be a multiple of 16", fn, (long long)N);
  AO_REQUIRE(Kc <= (1ll << 17), "%s: Kc=%lld above 2^17 could leave the int32 accumulator's range", fn, (long long)Kc);
  AO_REQUIRE(a_t == 0 || M % 16 == 0, "%s: a in [Kc][M] needs M=%lld, its contiguous dimension, a multiple of 16", fn, (long long)M);
  AO_REQUIRE((a_t == 1 && b_t == 1) || Kc % 16 == 0, "%s: an operand with the contraction innermost needs Kc=%lld a multiple of 16", fn, (long long)Kc);
  AO_REQUIRE(M <= (1ll << 22) && N <= (1ll << 22), "%s: M=%lld N=%lld too large (both <= 2^22)", fn, (long long)M, (long long)N);
  return AO_OK;
}

template <bool AT, bool BT>
void launch_train_mm(const TrainMmArgs& p, hipStream_t stream) {
  ao::launch(int8_train_mm_kernel<AT, BT>, dim3((unsigned)((p.N + kMmTile - 1) / kMmTile), (unsigned)((p.M + kMmTile - 1) / kMmTile)), dim3(256), 0, stream, p);
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int64_t ao_int8_train_quantize_workspace_bytes(int64_t R, int64_t C) {
  if (R <= 0 || C <= 0) return 0;
  const int64_t strips = (R + kStripRows - 1) / kStripRows, chunks = (C + kAmaxChunk - 1) / kAmaxChunk;
  return (((strips * C + R * chunks) * 2 + 15) / 16) * 16;
}

extern "C" int ao_int8_train_quantize(const uint16_t* x, int8_t* q_row, uint16_t* s_row, int8_t* q_col, uint16_t* s_col, void* workspace, int64_t R,
                                      int64_t C, float eps, int sr, int64_t sr_seed, int64_t sr_offset, void* stream) {
  if (int rc = check_rows(__func__, R, C, 16)) return rc;
  AO_REQUIRE(C <= (1ll << 24), "%s: C=%lld too large", __func__, (long long)C);
  AO_REQUIRE((q_row == nullptr) == (s_row == nullptr) && (q_col == nullptr) == (s_col == nullptr),
             "%s: the codes and the scales of a direction come together (q_row with s_row, q_col with s_col)", __func__);
  AO_REQUIRE(q_row != nullptr || q_col != nullptr, "%s: neither the row nor the column cast is asked for", __func__);
  AO_REQUIRE(sr == 0 || q_row != nullptr, "%s: stochastic rounding is the row cast's, and no row cast is asked for", __func__);
  AO_REQUIRE(eps >= 0.f, "%s: eps=%g must not be negative", __func__, (double)eps);
  if (R == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(q_row, 16) && aligned_to(q_col, 16) && aligned_to(s_col, 16) && aligned_to(workspace, 16),
             "%s: x, q_row, q_col, s_col and workspace must be 16-byte aligned", __func__);
  const SrKey key{sr != 0, (uint32_t)(uint64_t)sr_seed, (uint32_t)((uint64_t)sr_seed >> 32), (uint32_t)(uint64_t)sr_offset, (uint32_t)((uint64_t)sr_offset >> 32)};
  hipStream_t st = (hipStream_t)stream;
  if (q_col == nullptr) {
    const int64_t per_thread = ((C >> 4) + kRowThreads - 1) / kRowThreads;
    auto go = [&](auto np) {
      ao::launch(int8_train_rows_kernel<decltype(np)::value>, dim3((unsigned)R), dim3(kRowThreads), 0, st, x, q_row, s_row, (int)C, eps, key);
    };
    if (per_thread <= 1) go(std::integral_constant<int, 1>{});
    else if (per_thread <= 2) go(std::integral_constant<int, 2>{});
    else if (per_thread <= 4) go(std::integral_constant<int, 4>{});
    else go(std::integral_constant<int, 0>{});
    AO_LAUNCH_CHECK("int8_train_rows_kernel launch");
    return AO_OK;
  }
  AO_REQUIRE_PTR(workspace);
  const int64_t strips = (R + kStripRows - 1) / kStripRows, chunks = (C + kAmaxChunk - 1) / kAmaxChunk;
  uint16_t* colpart = static_cast<uint16_t*>(workspace);
  uint16_t* rowpart = q_row != nullptr ? colpart + strips * C : nullptr;
  ao::launch(int8_train_amax_kernel, dim3((unsigned)strips, (unsigned)chunks), dim3(256), 0, st, x, colpart, rowpart, (int)R, (int)C);
  AO_LAUNCH_CHECK("int8_train_amax_kernel launch");
  ao::launch(int8_train_col_scale_kernel, dim3((unsigned)((C / 2 + 255) / 256)), dim3(256), 0, st, (const uint16_t*)colpart, (int)strips, (int)C, s_col);
  AO_LAUNCH_CHECK("int8_train_col_scale_kernel launch");
  ao::launch(int8_train_cast_kernel, dim3((unsigned)strips, (unsigned)((C + kCastCols - 1) / kCastCols)), dim3(256), 0, st, x, (const uint16_t*)s_col,
             (const uint16_t*)rowpart, (int)chunks, q_row, s_row, q_col, (int)R, (int)C, eps, key);
  AO_LAUNCH_CHECK("int8_train_cast_kernel launch");
  return AO_OK;
}

extern "C" int ao_int8_train_mm_fits(int64_t M, int64_t N, int64_t Kc, int a_t, int b_t) {
  return train_mm_check_shape(__func__, M, N, Kc, a_t, b_t) == AO_OK ? 1 : 0;
}

extern "C" const char* ao_int8_train_mm_kernel_name(int a_t, int b_t) {
  static const char* const names[4] = {"int8_train_mm_kernel<0,0>", "int8_train_mm_kernel<0,1>", "int8_train_mm_kernel<1,0>", "int8_train_mm_kernel<1,1>"};
  return ((a_t | b_t) & ~1) ? "" : names[a_t * 2 + b_t];
}

extern "C" int ao_int8_train_mm(const int8_t* a, const int8_t* b, const uint16_t* sa, const uint16_t* sb, uint16_t* out, int64_t M, int64_t N, int64_t Kc,
                                int a_t, int b_t, void* stream) {
  if (int rc = train_mm_check_shape(__func__, M, N, Kc, a_t, b_t)) return rc;
  if (M == 0 || N == 0) return AO_OK;
  AO_REQUIRE_PTR(a);
  AO_REQUIRE_PTR(b);
  AO_REQUIRE_PTR(sa);
  AO_REQUIRE_PTR(sb);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(sb, 16) && aligned_to(out, 16), "%s: a, b, sb and out must be 16-byte aligned", __func__);
  const TrainMmArgs p{a, b, sa, sb, out, (int)M, (int)N, (int)Kc};
  hipStream_t st = (hipStream_t)stream;
  if (!a_t && !b_t) launch_train_mm<false, false>(p, st);
  else if (!a_t && b_t) launch_train_mm<false, true>(p, st);
  else if (a_t && !b_t) launch_train_mm<true, false>(p, st);
  else launch_train_mm<true, true>(p, st);
  AO_LAUNCH_CHECK("int8_train_mm_kernel launch");
  return AO_OK;
}
