// Codebook (k-means) weights (torchao/prototype/quantization/codebook) on gfx950: the fused Lloyd step of the calibration, the nibble
// packing, the dequantize, and a bf16 x codebook linear that gathers whole MFMA operand fragments out of a table in LDS.  The format and
// the arithmetic are stated once, in quant_math.h ("Codebook"); DESIGN.md 4.35 has the measurements.
//
//   codebook_assign_kernel<D, K, LLOYD>: replaces one iteration of fit_kmeans (codebook_ops.py:290-316: an addmm that writes a
//     [rows, k] fp32 score matrix, an argmax over it, an index_reduce_ whose atomics funnel every row onto k table rows) and the chunk
//     loop of quantize_codebook (:74-90).  The fp32 table [K][D] and the half norms h sit in LDS.  A lane keeps B rows of the data in
//     registers (B = 4 at D >= 4, 8 below) and walks the table once: every lane of a wave reads the SAME entry (an LDS broadcast, no bank
//     conflict), so one entry read of D / 4 + 1 LDS instructions feeds B x D v_fma_f32 and B compare-and-keep steps.  With one row a
//     lane an entry of D = 8 would cost 3 LDS reads per 8 FMAs and the loop would wait on LDS; with four it is 3 per 32, and 32 + 32 data
//     and bookkeeping registers keep 8 waves a SIMD.  No score is ever written.  A tile is 256 B rows, row b 256 + t of the tile to lane
//     t (coalesced); workgroups walk the tiles with the stride of the grid.
//     LLOYD: each row is then added to its entry's D sums and count in LDS (ds_add_f32 / ds_add_u32: no global atomics), and the
//     workgroup writes its [K][D] sums and [K] counts to its own slice of the workspace.  The order of the LDS adds inside a workgroup
//     is free, so the low bits of a sum can differ between launches, like index_reduce_ on a GPU.
//   codebook_reduce_kernel: thread (entry j, element i) adds the workgroups' partial sums IN WORKGROUP ORDER and writes sum / count; an
//     entry without a member keeps its old centroid's bits (index_reduce_(include_self=False) on a clone).
//   codebook_pack_u4_kernel: two codes a byte, the even one in the low nibble.
//   codebook_dequantize_kernel<D, U4>: the tensor as a flat run of pieces of 8 weights (sb % 8 == 0: a piece has one scale; the codes and
//     scales of a [N][K] tensor are flat runs too, so the kernel knows nothing of rows), the bf16 table in LDS, one 16-byte store a
//     piece; scale blocks off the 8 grid take the same kernel's element-wise path with 2-byte stores.
//   codebook_stream_kernel<D, U4, MT, WAVES>: the weight-streaming linear on the plan of two_form_route.h.  A workgroup owns 16 columns
//     and splits K over its waves in 128-k steps; lane (column l & 15, group kq) takes the 32 k at 32 kq of a step: 32 / D codes (32 to
//     2 bytes), one scale (sb % 32 == 0).  The bf16 table (k D 2 bytes, at most 4 KiB) is in LDS and an MFMA operand -- 8 consecutive k of
//     one row -- is gathered from it: one ds_read_b128 at 16 code for D = 8, two ds_read_b64 for D = 4, four ds_read_b32 for D = 2,
//     eight ds_read_u16 for D = 1; then 8 multiplies by the scale and 4 v_cvt_pk_bf16_f32 in front of v_mfma_f32_16x16x32_bf16.  The
//     partial tiles meet in LDS in wave order.  There is no LDS-tiled form: above the seam the route says "not fused".
#include "common.h"
#include "quant_math.h"
#include "two_form_route.h"

#include <algorithm>

namespace ao {
namespace {

// ---- the format -----------------------------------------------------------------------------------------------------------------------
const char* codebook_format_reason(int d, int k) {
  if (d != 1 && d != 2 && d != 4 && d != 8) return "d must be 1, 2, 4 or 8";
  if (k != 16 && k != 256) return "k must be 16 (uint4 codes) or 256 (uint8 codes)";
  return nullptr;
}

const char* codebook_tensor_reason(int64_t N, int64_t K, int d, int k, int64_t sb) {
  if (const char* why = codebook_format_reason(d, k)) return why;
  if (N < 0 || K < 1) return "N >= 0 and K >= 1 are required";
  if (sb < 1 || K % sb != 0 || sb % d != 0) return "sb must divide K and be a multiple of d";
  if (k == 16 && (K / d) % 2 != 0) return "K / d must be even for uint4 codes (two a byte)";
  if (N >= (1ll << 31) || K >= (1ll << 31) || N * K >= (1ll << 40)) return "N, K < 2^31 and N K < 2^40 are required";
  return nullptr;
}

template <typename F>
int with_format(int d, int k, F&& f) {
  auto with_k = [&](auto dd) {
    if (k == 16) return f(dd, std::integral_constant<int, 16>{});
    return f(dd, std::integral_constant<int, 256>{});
  };
  switch (d) {
    case 1: return with_k(std::integral_constant<int, 1>{});
    case 2: return with_k(std::integral_constant<int, 2>{});
    case 4: return with_k(std::integral_constant<int, 4>{});
    default: return with_k(std::integral_constant<int, 8>{});
  }
}

// ---- assignment and the Lloyd step -------------------------------------------------------------------------------------------------------
constexpr int cb_rows_per_lane(int d) { return d >= 4 ? 4 : 8; }
constexpr int kMaxGroups = 1024;  // workgroups of a launch (4 a CU): the reduce adds at most this many partials per entry

int64_t cb_tiles(int64_t n, int d) { return (n + 256 * cb_rows_per_lane(d) - 1) / (256 * cb_rows_per_lane(d)); }
int64_t cb_groups(int64_t n, int d) { return std::min<int64_t>(cb_tiles(n, d), kMaxGroups); }

struct CbAssignArgs {
  const float* x;      // [n][D]
  const float* table;  // [K][D]
  uint8_t* codes;      // [n] or null
  float* part_sum;     // [groups][K][D]
  int* part_cnt;       // [groups][K]
  int64_t n, tiles;
};

template <int D>
__device__ __forceinline__ void cb_load_row(const float* p, float (&v)[D]) {
  if constexpr (D == 8) {
    const f32x4 a = reinterpret_cast<const f32x4*>(p)[0], b = reinterpret_cast<const f32x4*>(p)[1];
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  } else if constexpr (D == 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
  } else if constexpr (D == 2) {
    const f32x2 a = *reinterpret_cast<const f32x2*>(p);
    v[0] = a.x, v[1] = a.y;
  } else {
    v[0] = *p;
  }
}

template <int D, int K, bool LLOYD>
__global__ __launch_bounds__(256) void codebook_assign_kernel(CbAssignArgs p) {
  constexpr int B = cb_rows_per_lane(D);
  __shared__ __attribute__((aligned(16))) float tab[K * D];
  __shared__ float hn[K];
  __shared__ float sum[LLOYD ? K * D : 1];
  __shared__ int cnt[LLOYD ? K : 1];
  const int tid = threadIdx.x;
  for (int i = tid; i < K * D; i += 256) {
    tab[i] = p.table[i];
    if (LLOYD) sum[i] = 0.f;
  }
  __syncthreads();
  for (int j = tid; j < K; j += 256) {
    hn[j] = codebook_half_norm(tab + j * D, D);
    if (LLOYD) cnt[j] = 0;
  }
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    float x[B][D], best[B];
    int code[B];
    int64_t row[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      row[b] = (tile * B + b) * 256 + tid;
      cb_load_row<D>(p.x + (row[b] < p.n ? row[b] : 0) * D, x[b]);  // (rows past n walk row 0 and store nothing)
      best[b] = -__builtin_inff();
      code[b] = -1;
    }
#pragma unroll 2
    for (int j = 0; j < K; ++j) {
      float c[D];
      cb_load_row<D>(tab + j * D, c);
      const float h = hn[j];
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const float s = codebook_score<D>(x[b], c, h);
        if (s > best[b]) best[b] = s, code[b] = j;  // strict: the lowest index of equal scores stays; a NaN never enters
      }
    }
    bool unset = false;
#pragma unroll
    for (int b = 0; b < B; ++b) unset |= code[b] < 0;
    if (unset) {  // rare: no score of a row was above -inf -- its lowest entry whose score is not NaN, 0 if there is none
      for (int j = 0; j < K; ++j) {
        float c[D];
        cb_load_row<D>(tab + j * D, c);
#pragma unroll
        for (int b = 0; b < B; ++b) {
          const float s = codebook_score<D>(x[b], c, hn[j]);
          if (code[b] == -1 && s == s) code[b] = j;
        }
      }
#pragma unroll
      for (int b = 0; b < B; ++b) code[b] = max(code[b], 0);
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      if (row[b] < p.n) {
        if (p.codes != nullptr) p.codes[row[b]] = (uint8_t)code[b];
        if (LLOYD) {
#pragma unroll
          for (int i = 0; i < D; ++i) atomicAdd(&sum[code[b] * D + i], x[b][i]);
          atomicAdd(&cnt[code[b]], 1);
        }
      }
    }
  }
  if (LLOYD) {
    __syncthreads();
    for (int i = tid; i < K * D; i += 256) p.part_sum[(size_t)blockIdx.x * (K * D) + i] = sum[i];
    for (int j = tid; j < K; j += 256) p.part_cnt[(size_t)blockIdx.x * K + j] = cnt[j];
  }
}

__global__ __launch_bounds__(256) void codebook_reduce_kernel(const float* part_sum, const int* part_cnt, int groups, const float* old_table,
                                                              float* new_table, int* counts, int k, int d) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= k * d) return;
  const int j = e / d;
  int c = 0;
  float s = 0.f;
  for (int g = 0; g < groups; ++g) {  // workgroup order: the same partials give the same bits
    c += part_cnt[(size_t)g * k + j];
    s += part_sum[(size_t)g * (k * d) + e];
  }
  new_table[e] = c > 0 ? s / (float)c : old_table[e];
  if (e == j * d) counts[j] = c;
}

__global__ __launch_bounds__(256) void codebook_pack_u4_kernel(const uint16_t* codes, uint8_t* packed, int64_t pairs) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= pairs) return;
  const uint32_t two = codes[t];  // code 2 t in the low byte
  packed[t] = (uint8_t)((two & 15u) | ((two >> 4) & 0xF0u));
}

// ---- the decode ------------------------------------------------------------------------------------------------------------------------------
// code q of a little-endian run of codes of CBITS bits (uint4: block 2 i in the low nibble of byte i); q is a constant after unrolling
template <int CBITS>
__device__ __forceinline__ uint32_t cb_code(const uint32_t* c, int q) {
  const int off = q * CBITS;
  return (c[off >> 5] >> (off & 31)) & ((1u << CBITS) - 1u);
}

// the 8 weights of fragment f of such a run (codes 8 / D f .. 8 / D (f + 1) - 1): table entries out of LDS, times the scale, as 8 bf16
template <int D, int CBITS>
__device__ __forceinline__ u32x4 cb_fragment(const char* tab, const uint32_t* c, int f, float s) {
  uint32_t r[4];
  if constexpr (D == 8) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(tab + cb_code<CBITS>(c, f) * 16);
    r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
  } else if constexpr (D == 4) {
    const u32x2 a = *reinterpret_cast<const u32x2*>(tab + cb_code<CBITS>(c, 2 * f) * 8);
    const u32x2 b = *reinterpret_cast<const u32x2*>(tab + cb_code<CBITS>(c, 2 * f + 1) * 8);
    r[0] = a.x, r[1] = a.y, r[2] = b.x, r[3] = b.y;
  } else if constexpr (D == 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = *reinterpret_cast<const uint32_t*>(tab + cb_code<CBITS>(c, 4 * f + i) * 4);
  } else {
    const uint16_t* t16 = reinterpret_cast<const uint16_t*>(tab);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (uint32_t)t16[cb_code<CBITS>(c, 8 * f + 2 * i)] | ((uint32_t)t16[cb_code<CBITS>(c, 8 * f + 2 * i + 1)] << 16);
  }
  return u32x4{codebook_decode2(r[0], s), codebook_decode2(r[1], s), codebook_decode2(r[2], s), codebook_decode2(r[3], s)};
}

// the bf16 table into LDS, a dword a thread a turn (k D is even)
__device__ __forceinline__ void cb_stage_table(char* tab, const uint16_t* codebook, int words, int threads) {
  for (int i = threadIdx.x; i < words; i += threads) reinterpret_cast<uint32_t*>(tab)[i] = reinterpret_cast<const uint32_t*>(codebook)[i];
}

// ---- dequantize ---------------------------------------------------------------------------------------------------------------------------
constexpr int kDequantTurns = 8;  // pieces a thread: the 4 KiB table is staged once per 32 KiB of output

struct CbDequantArgs {
  const uint8_t* codes;
  const uint16_t* codebook;
  const uint16_t* scales;
  uint16_t* out;
  int64_t total;  // N K
  int64_t sb;
  int k;
};

template <int D, bool U4>
__global__ __launch_bounds__(256) void codebook_dequantize_kernel(CbDequantArgs p) {
  constexpr int CBITS = U4 ? 4 : 8, BITS = (8 / D) * CBITS;  // the codes of a piece: 64, 32, 16, 8 or 4 bits
  __shared__ __attribute__((aligned(16))) char tab[4096];
  cb_stage_table(tab, p.codebook, p.k * D / 2, 256);
  __syncthreads();
  const int64_t pieces = (p.total + 7) >> 3;
  const bool whole = (p.sb & 7) == 0;  // (then 8 | K too, and N K is a whole number of pieces)
  for (int it = 0; it < kDequantTurns; ++it) {
    const int64_t t = ((int64_t)blockIdx.x * kDequantTurns + it) * 256 + threadIdx.x;
    if (t >= pieces) return;
    if (whole) {
      uint32_t c[2] = {0u, 0u};
      if constexpr (BITS == 64) {
        const u32x2 v = reinterpret_cast<const u32x2*>(p.codes)[t];
        c[0] = v.x, c[1] = v.y;
      } else if constexpr (BITS == 32) {
        c[0] = reinterpret_cast<const uint32_t*>(p.codes)[t];
      } else if constexpr (BITS == 16) {
        c[0] = reinterpret_cast<const uint16_t*>(p.codes)[t];
      } else if constexpr (BITS == 8) {
        c[0] = p.codes[t];
      } else {
        c[0] = (p.codes[t >> 1] >> (4 * (int)(t & 1))) & 15u;
      }
      const float s = bf16_lo_to_f32(p.scales[(t * 8) / p.sb]);
      reinterpret_cast<u32x4*>(p.out)[t] = cb_fragment<D, CBITS>(tab, c, 0, s);
    } else {
      const uint16_t* t16 = reinterpret_cast<const uint16_t*>(tab);
      for (int64_t e = t * 8; e < t * 8 + 8 && e < p.total; ++e) {
        const int64_t blk = e / D;
        const uint32_t code = U4 ? (p.codes[blk >> 1] >> (4 * (int)(blk & 1))) & 15u : p.codes[blk];
        p.out[e] = f32_to_bf16_bits(bf16_lo_to_f32(t16[code * D + (int)(e % D)]) * bf16_lo_to_f32(p.scales[e / p.sb]));
      }
    }
  }
}

// ---- the linear: the route -----------------------------------------------------------------------------------------------------------------
// The stream form up to these rows, by block width; beyond, dequantize + bf16 GEMM (kernel 0).  Started from the NF4 linear's seam and
// fitted on the Llama-3-8B five shapes (profiles/codebook.jsonl, its four "fit" lines: tools/bench_codebook.py --sweep, uint8 codes, the
// fused form forced and dequantize + F.linear at M = 1 .. 256, weights from HBM, three windows a cell, the five shapes summed over every
// swept M per candidate seam; then the five shapes at one M, fused against dequantize + F.linear):
//   d = 1  3063.5 us at 33, 3064.3 at 48, 3092.0 at 64, 3218.9 at 65; at 48 rows 232.7 against 232.0, at 64 rows 268.7 against 241.0
//   d = 2  2787.7 at 48, 2789.3 at 64, 2831.5 at 65;                   at 48 rows 201.7 against 225.3, at 64 rows 236.3 against 234.8
//   d = 4  2778.6 at 64, 2784.0 at 48, 2812.7 at 65;                   at 64 rows 236.2 against 241.7, at 65 rows 279.1 against 244.9
//   d = 8  2772.0 at 64, 2781.4 at 48, 2799.7 at 65;                   at 64 rows 233.7 against 243.2, at 65 rows 275.5 against 247.7
// The narrow blocks pay more gathers a fragment (eight and four) and lose at 64 rows; 33 and 48 are even for d = 1 and 48 keeps the rows
// where the fused form still wins.  Not fitted: a seam per shape (at 64 rows the wide-N shapes are behind, the square ones ahead).
constexpr int cb_stream_max_rows(int d) { return d <= 2 ? AO_CODEBOOK_LINEAR_STREAM_MAX_M_NARROW : AO_CODEBOOK_LINEAR_STREAM_MAX_M; }

thread_local int g_form = 0;  // ao_codebook_linear_set_form: 0 the product route, 1 the stream form at any M

// what codebook_stream_kernel takes: a lane's 32 k inside one scale block, 32-bit element counts, the scale index by a multiply
const char* codebook_linear_reason(int64_t M, int64_t N, int64_t K, int d, int k, int64_t sb) {
  if (const char* why = codebook_tensor_reason(N, K, d, k, sb)) return why;
  if (M < 0 || N < 1) return "M >= 0 and N >= 1 are required";
  if (K % 32 != 0 || sb % 32 != 0) return "the fused form takes K and sb that are multiples of 32 (a lane's 32 k share one scale)";
  if (K > (1ll << 20)) return "the fused form takes K <= 2^20";
  if (M >= (1ll << 31) || N * K >= (1ll << 31) || M * K >= (1ll << 31) || M * N >= (1ll << 40)) return "x and W must hold fewer than 2^31 elements";
  return nullptr;
}

// kernel 1: codebook_stream_kernel; 0: not fused (dequantize, then multiply) -- above the seam, and for shapes the kernel does not take
TwoFormRoute codebook_route(int64_t M, int64_t N, int64_t K, int d, int k, int64_t sb) {
  if (codebook_linear_reason(M, N, K, d, k, sb) != nullptr) return TwoFormRoute{};
  if (g_form == 0 && M > cb_stream_max_rows(d)) return TwoFormRoute{};
  return two_form_route(1, M, N, K, 0);
}

struct CbLinearArgs {
  const uint16_t* x;         // bf16 [M][K]
  const uint8_t* codes;      // [N][K / D] bytes, or [N][K / (2 D)]
  const uint16_t* codebook;  // bf16 [k][D]
  const uint16_t* scales;    // bf16 [N][K / sb]
  uint16_t* out;             // bf16 [M][N]
  int M, N, K;
  int k;
  int sblocks;     // K / sb
  uint32_t magic;  // floor(2^32 / (sb / 32)) + 1: (k / 32) / (sb / 32) == umulhi(k / 32, magic) while (K / 32)^2 < 2^32; 0: sb == 32
};

__device__ __forceinline__ f32x4 mfma_bf16(const u32x4& a, const u32x4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// the CB bytes of codes of a lane's 32 k (CB = 32, 16, 8, 4 or 2; aligned to CB: rows are multiples of CB long)
template <int CB>
__device__ __forceinline__ void cb_load_codes(const uint8_t* p, uint32_t (&c)[(CB + 3) / 4]) {
  if constexpr (CB == 32) {
    const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)), b = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p) + 1);
    c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = a.w, c[4] = b.x, c[5] = b.y, c[6] = b.z, c[7] = b.w;
  } else if constexpr (CB == 16) {
    const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = a.w;
  } else if constexpr (CB == 8) {
    const u32x2 a = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
    c[0] = a.x, c[1] = a.y;
  } else if constexpr (CB == 4) {
    c[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
  } else {
    c[0] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p));
  }
}

constexpr int kChunk = 4;  // 128-k steps a wave requests at once

template <int D, bool U4, int MT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void codebook_stream_kernel(CbLinearArgs p) {
  constexpr int CBITS = U4 ? 4 : 8, CB = 4 * CBITS / D, CW = (CB + 3) / 4;
  __shared__ f32x4 red[WAVES][MT][64];
  __shared__ __attribute__((aligned(16))) char tab[4096];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kq = lane >> 4;
  cb_stage_table(tab, p.codebook, p.k * D / 2, 64 * WAVES);
  lds_barrier();
  const int n = blockIdx.x * 16 + (lane & 15);
  const int m0 = blockIdx.y * 16 * MT;
  const int runs = p.K >> 5;  // 32 | K: the 32 k of a lane lie inside K or outside; outside, the row's first 32 are read and both operands zeroed
  const int ksteps = (runs + 3) >> 2;
  const int ks0 = (ksteps * wave) / WAVES, ks1 = (ksteps * (wave + 1)) / WAVES;
  // columns past N read the last row (never stored)
  const int nr = min(n, p.N - 1);
  const uint8_t* crow = p.codes + (size_t)nr * runs * CB;
  const uint16_t* srow = p.scales + (size_t)nr * p.sblocks;
  struct Stage {
    uint32_t c[CW];
    uint32_t s;
  };
  auto issue = [&](Stage (&st)[kChunk], int step) {
#pragma unroll
    for (int d = 0; d < kChunk; ++d) {
      const int run = (step + d) * 4 + kq;
      const int r = run < runs ? run : 0;
      cb_load_codes<CB>(crow + (size_t)r * CB, st[d].c);
      st[d].s = srow[p.magic != 0u ? __umulhi((uint32_t)r, p.magic) : (uint32_t)r];
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
        const int run = (step + d) * 4 + kq;
        const bool v = run < runs;
        const u32x4 z = {0u, 0u, 0u, 0u};
        const float s = bf16_lo_to_f32(cur[d].s);
        u32x4 w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = cb_fragment<D, CBITS>(tab, cur[d].c, i, s);
        if (!v) w[0] = w[1] = w[2] = w[3] = z;  // (not 0 x scale: a scale may be NaN)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const u32x4* xp = reinterpret_cast<const u32x4*>(p.x + arow[mt] * p.K + (v ? run * 32 : 0));
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

int check_rows_nd(const char* fn, int64_t n, int d, int k) {
  const char* why = codebook_format_reason(d, k);
  AO_REQUIRE(why == nullptr, "%s: %s (d=%d k=%d)", fn, why, d, k);
  AO_REQUIRE(n >= 0 && n < (1ll << 40), "%s: n=%lld must be in [0, 2^40)", fn, (long long)n);
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_codebook_assign(const float* x, const float* table, uint8_t* codes, int64_t n, int d, int k, void* stream) {
  if (int rc = check_rows_nd(__func__, n, d, k)) return rc;
  if (n == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(table);
  AO_REQUIRE_PTR(codes);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(table, 4), "%s: x must be 16-byte and table 4-byte aligned", __func__);
  const int64_t tiles = cb_tiles(n, d);
  const CbAssignArgs a{x, table, codes, nullptr, nullptr, n, tiles};
  with_format(d, k, [&](auto dd, auto kk) {
    ao::launch(codebook_assign_kernel<decltype(dd)::value, decltype(kk)::value, false>, dim3((unsigned)cb_groups(n, d)),
               dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return 0;
  });
  AO_LAUNCH_CHECK("codebook_assign_kernel launch");
  return AO_OK;
}

extern "C" int64_t ao_codebook_lloyd_workspace_bytes(int64_t n, int d, int k) {
  if (codebook_format_reason(d, k) != nullptr || n < 0 || n >= (1ll << 40)) return -1;
  return cb_groups(n, d) * k * (d + 1) * 4;
}

extern "C" int ao_codebook_lloyd_step(const float* x, const float* table, float* new_table, int32_t* counts, uint8_t* codes, void* workspace,
                                      int64_t workspace_bytes, int64_t n, int d, int k, void* stream) {
  if (int rc = check_rows_nd(__func__, n, d, k)) return rc;
  const int64_t groups = cb_groups(n, d), need = groups * k * (d + 1) * 4;
  AO_REQUIRE(workspace_bytes >= need, "%s: the workspace holds %lld bytes, ao_codebook_lloyd_workspace_bytes(n, d, k) = %lld are needed", __func__,
             (long long)workspace_bytes, (long long)need);
  AO_REQUIRE_PTR(table);
  AO_REQUIRE_PTR(new_table);
  AO_REQUIRE_PTR(counts);
  if (n > 0) {
    AO_REQUIRE_PTR(x);
    AO_REQUIRE_PTR(workspace);
  }
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(table, 4) && aligned_to(new_table, 4) && aligned_to(counts, 4) && aligned_to(workspace, 4),
             "%s: x must be 16-byte, table, new_table, counts and workspace 4-byte aligned", __func__);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part_sum = static_cast<float*>(workspace);
  int* part_cnt = reinterpret_cast<int*>(part_sum + groups * k * d);
  if (n > 0) {
    const CbAssignArgs a{x, table, codes, part_sum, part_cnt, n, cb_tiles(n, d)};
    with_format(d, k, [&](auto dd, auto kk) {
      ao::launch(codebook_assign_kernel<decltype(dd)::value, decltype(kk)::value, true>, dim3((unsigned)groups), dim3(256), 0, st, a);
      return 0;
    });
    AO_LAUNCH_CHECK("codebook_assign_kernel (Lloyd) launch");
  }
  // (no rows: no partials, every entry keeps its centroid and a count of 0)
  ao::launch(codebook_reduce_kernel, dim3((unsigned)((k * d + 255) / 256)), dim3(256), 0, st, part_sum, part_cnt, (int)groups, table, new_table,
             counts, k, d);
  AO_LAUNCH_CHECK("codebook_reduce_kernel launch");
  return AO_OK;
}

extern "C" int ao_codebook_pack_u4(const uint8_t* codes, uint8_t* packed, int64_t n, void* stream) {
  AO_REQUIRE(n >= 0 && n % 2 == 0 && n < (1ll << 40), "%s: n=%lld must be even (two codes a byte) and below 2^40", __func__, (long long)n);
  if (n == 0) return AO_OK;
  AO_REQUIRE_PTR(codes);
  AO_REQUIRE_PTR(packed);
  AO_REQUIRE(aligned_to(codes, 2), "%s: codes must be 2-byte aligned", __func__);
  ao::launch(codebook_pack_u4_kernel, dim3((unsigned)((n / 2 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
             reinterpret_cast<const uint16_t*>(codes), packed, n / 2);
  AO_LAUNCH_CHECK("codebook_pack_u4_kernel launch");
  return AO_OK;
}

extern "C" int ao_codebook_dequantize(const uint8_t* codes, const uint16_t* codebook, const uint16_t* scales, uint16_t* out, int64_t N, int64_t K,
                                      int d, int k, int64_t sb, void* stream) {
  const char* why = codebook_tensor_reason(N, K, d, k, sb);
  AO_REQUIRE(why == nullptr, "%s: %s (N=%lld K=%lld d=%d k=%d sb=%lld)", __func__, why, (long long)N, (long long)K, d, k, (long long)sb);
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(codes);
  AO_REQUIRE_PTR(codebook);
  AO_REQUIRE_PTR(scales);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(codes, 8) && aligned_to(codebook, 4) && aligned_to(scales, 2) && aligned_to(out, 16),
             "%s: codes must be 8-byte, codebook 4-byte, scales 2-byte and out 16-byte aligned", __func__);
  const int64_t pieces = (N * K + 7) / 8, grid = (pieces + 256 * kDequantTurns - 1) / (256 * kDequantTurns);
  const CbDequantArgs a{codes, codebook, scales, out, N * K, sb, k};
  with_format(d, k, [&](auto dd, auto kk) {
    ao::launch(codebook_dequantize_kernel<decltype(dd)::value, decltype(kk)::value == 16>, dim3((unsigned)grid), dim3(256), 0,
               static_cast<hipStream_t>(stream), a);
    return 0;
  });
  AO_LAUNCH_CHECK("codebook_dequantize_kernel launch");
  return AO_OK;
}

extern "C" int ao_codebook_linear_fits(int64_t M, int64_t N, int64_t K, int d, int k, int64_t sb) {
  const char* why = codebook_linear_reason(M, N, K, d, k, sb);
  if (why != nullptr) set_error("%s: %s (M=%lld N=%lld K=%lld d=%d k=%d sb=%lld)", __func__, why, (long long)M, (long long)N, (long long)K, d, k, (long long)sb);
  return why == nullptr ? 1 : 0;
}

extern "C" int ao_codebook_linear_route(int64_t M, int64_t N, int64_t K, int d, int k, int64_t sb, int32_t* out, int cap) {
  return route_export(__func__, codebook_route(M, N, K, d, k, sb), out, cap);
}

extern "C" const char* ao_codebook_linear_kernel_name(int64_t M, int64_t N, int64_t K, int d, int k, int64_t sb) {
  return codebook_route(M, N, K, d, k, sb).kernel == 1 ? "codebook_stream_kernel" : "not fused";
}

extern "C" int ao_codebook_linear_set_form(int form) {
  AO_REQUIRE(form == 0 || form == 1, "%s: form must be 0 (route) or 1 (stream): there is no tiled form, got %d", __func__, form);
  return set_forced_form(__func__, form, g_form);
}

extern "C" int ao_codebook_linear(const uint16_t* x, const uint8_t* codes, const uint16_t* codebook, const uint16_t* scales, uint16_t* out, int64_t M,
                                  int64_t N, int64_t K, int d, int k, int64_t sb, void* stream) {
  const char* why = codebook_linear_reason(M, N, K, d, k, sb);
  AO_REQUIRE(why == nullptr, "%s: %s (M=%lld N=%lld K=%lld d=%d k=%d sb=%lld)", __func__, why, (long long)M, (long long)N, (long long)K, d, k,
             (long long)sb);
  AO_REQUIRE_PTR(codes);
  AO_REQUIRE_PTR(codebook);
  AO_REQUIRE_PTR(scales);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(codes, 16) && aligned_to(codebook, 4) && aligned_to(scales, 2) && aligned_to(out, 2),
             "%s: x and codes must be 16-byte, codebook 4-byte, scales and out 2-byte aligned", __func__);
  const TwoFormRoute r = codebook_route(M, N, K, d, k, sb);
  AO_REQUIRE(r.kernel == 1, "%s: M=%lld is not fused (more than %d rows, or more than 65535 grid rows): dequantize, then multiply", __func__,
             (long long)M, cb_stream_max_rows(d));
  const int64_t sb32 = sb / 32;
  const CbLinearArgs a{x, codes, codebook, scales, out, (int)M, (int)N, (int)K, k, (int)(K / sb), sb32 == 1 ? 0u : (uint32_t)((1ull << 32) / (uint64_t)sb32 + 1)};
  return with_format(d, k, [&](auto dd, auto kk) {
    return launch_stream_form<false>("codebook_stream_kernel", "codebook_stream_kernel launch", r, a, static_cast<hipStream_t>(stream),
                                     [](auto mt, auto waves) {
                                       return codebook_stream_kernel<decltype(dd)::value, decltype(kk)::value == 16, decltype(mt)::value, decltype(waves)::value>;
                                     });
  });
}
