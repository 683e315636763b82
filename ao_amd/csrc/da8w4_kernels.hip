// W4A8 linears (torchao/prototype/quantization/int4: Int8DynamicActivationInt4WeightConfig, Int4OpaqueTensor.from_hp_da8w4, served there by a
// CPU-only kernel) on gfx950: int8 activation codes x 4-bit weight codes on the integer matrix pipe, an exact int32 sum inside a group.
//
// The arithmetic, every step ONE fp32 or bf16 operation rounded once, the divisions IEEE (the recorded fixture tests/golden/da8w4.npz is
// reproduced by exactly this chain):
//   range    mn = min(min, 0), mx = max(max, 0) over a weight group of g along K / over an activation row (token)
//   qparams  ASYMMETRIC, codes 0 .. Q (weight Q = 15, activation Q = 255), in bf16 TENSOR arithmetic:
//              s = max(bf16(bf16(mx - mn) / Q), bf16(eps));  zp = clamp(bf16(0 - rint(bf16(mn / s))), 0, Q)
//            SYMMETRIC activation: s = max(bf16(max(-mn, mx) / 127), eps), zp = 0, codes clamped to +-127
//            eps: 1e-6 for the weight (9.98e-7 as bf16), 2^-23 for the activation.  The scale is then stored as fp32, the zero-point as an integer.
//   code     q = clamp(rint(f32(v) * (1.0f / f32(s))) + zp, qmin, qmax) in fp32: the scale is widened BEFORE the reciprocal
//   linear   I_g[m][n] = sum_{k in group g} (qa[m][k] - za[m]) (qw[n][k] - zw[n][g]) in int32, exact (below 2^24);
//            acc = fma(f32(I_g), sw[n][g], acc) in fp32, g ascending (the stream form adds its waves' K shares in wave order);
//            y = bf16(f32(acc * sa[m]) + f32(bias[n])).  The reference multiplies by sa[m] inside the sum; here it is one multiply in the
//            epilogue (a named deviation).
//   decode   w = bf16((qw - zw) * s): exact.
// The device stores an ASYMMETRIC activation code as int8 qa - 128 and carries za - 128: the product does not change.
//
// The packed weight.  A row is cut into SUPERBLOCKS of 128 k = 64 bytes (K is padded with zero codes to a multiple of 128).  Byte
// b = 16 kq + 4 d + j of a superblock holds, in nibble t (bits 4 t .. 4 t + 3), the code of k = 64 t + 32 (d >> 1) + 8 kq + 4 (d & 1) + j.
// So a lane's 16-byte load (piece kq) is four dwords d, `(dword >> 4 t) & 0x0f0f0f0f` is four codes as four int8, and
//   the four dwords of plane t ARE lane group kq's operand of a v_mfma_i32_16x16x64_i8 over k = 64 t .. 64 t + 63 (g >= 64), matched by the two
//     8-byte runs 64 t + 8 kq and 64 t + 32 + 8 kq of the activation row in NATURAL order;
//   dwords 2 h, 2 h + 1 of plane t are its operand of a v_mfma_i32_16x16x32_i8 over k = 64 t + 32 h .. + 31 (g = 32: one instruction, one group).
// Nothing is shuffled on either side.  The MFMA runs on the RAW nibbles qw and the STORED int8 codes a (a = qa - 128 and za' = za - 128 when
// asymmetric, a = qa and za' = 0 when symmetric, so a - za' = qa - za): P_g = sum_k a qw, and expanding sum_k (a - za') (qw - zw) gives
//   I_g = P_g - zw sum_k a - za' sum_k (qw - zw),   one v_dot2_i32_i16 a register:
// the weight cast leaves (zw, sum_k (qw - zw)) as two int16 in a dword next to the fp32 scale (scale_and_zero [G][N][2]: group-major, so that
// four adjacent columns are two 16-byte loads), the activation cast leaves (-sum_k a, -za') per (row, group) (act_meta [M][G padded to 4]).
//
//   stream form  a workgroup owns 16 output columns and 16 rows; its waves take the 128-k steps in turn (whole groups), request up to four
//                steps ahead, unpack in registers; the activation rows are staged through LDS once a workgroup, 2048 k at a time; the fp32
//                partial tiles meet in LDS in wave order.
//   tiled form   128 x 64 output tiles, four waves of 64 x 32, K steps of 128, three LDS stages filled by global_load_lds: the activation
//                (16-byte pieces swizzled on the source side), the PACKED weight, and both operands' group metadata.  One int32 accumulator
//                set per group, folded into the fp32 set (v_dot2_i32_i16, v_cvt_f32_i32, v_fma_f32) at each group boundary.  W is the MFMA's A
//                operand, so a lane ends with four adjacent columns of one row.  72 KiB of LDS: two workgroups a CU, two waves a SIMD.
#include "common.h"
#include "lds_dma.h"
#include "quant_math.h"
#include "two_form_route.h"

#include <algorithm>

namespace ao {
namespace {

// The form seam: the stream form up to this many rows.  It started as a guess of 16 (the rows of one m-tile); fitted since on the Llama-3-8B o and
// gate shapes at g = 128 (profiles/da8w4_linear.jsonl: its "forms" and "fit" lines, tools/bench_da8w4_linear.py --sweep, both forms forced at
// M = 1 .. 256, weights from HBM): summed over the two shapes the stream form is ahead up to 64 rows (66.6 us against 75.1) and behind from 96
// (95.8 against 75.2); 65 .. 95 rows were not swept.  Per shape the seams differ: o stays ahead streamed to 128 rows, gate is behind from 48.
constexpr int kStreamMaxRows = AO_DA8W4_LINEAR_STREAM_MAX_M;

constexpr float kActEps = 1.1920928955078125e-07f;  // torch.finfo(torch.float32).eps, a bf16 value
constexpr float kWeightEps = 1e-6f;                 // rounded to bf16 where it meets the bf16 scale

typedef short i16x2 __attribute__((ext_vector_type(2)));

thread_local int g_form = 0;  // ao_da8w4_linear_set_form: 0 the route, 1 stream, 2 tile

__device__ __forceinline__ void da8w4_qparams(float mn, float mx, float qmax, float eps, float& s, float& zp) {
  s = fmaxf(round_bf16(round_bf16(mx - mn) / qmax), eps);
  zp = round_bf16(0.f - rintf(round_bf16(mn / s)));
  zp = fminf(fmaxf(zp, 0.f), qmax);
}
// P - zw * sum_a - c * za' on (zw, c) and (-sum_a, -za') as int16 pairs
__device__ __forceinline__ int da8w4_group_sum(uint32_t wmeta, uint32_t ameta, int p) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, wmeta), __builtin_bit_cast(i16x2, ameta), p, false);
}
// (the output element from the group sums: quant_math.h, da8w4_out)

// ---- the weight cast: a thread owns one 16-byte piece (row n, superblock sb, piece kq) = 8 weights of each of the superblock's four 32-k
// runs c = 2 t + h; the four lanes kq of a superblock meet by butterfly, the runs of a group of 64 / 128 in the lane itself --------------------
struct Da8w4WeightArgs {
  const uint16_t* w;  // bf16 [N][K]
  uint32_t* packed;   // [N][Kp / 8]
  float* sz;          // [G][N][2]: scale, then (zw, sum (q - zw)) as two int16
  int8_t* qzeros;     // [G][N]
  int16_t* comp;      // [G][N]
  int64_t pieces;     // N * Kp / 32
  int N, K, Kp, g;
};

__global__ __launch_bounds__(kRowThreads) void da8w4_quantize_weight_kernel(Da8w4WeightArgs p) {
  const int64_t id = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const bool live = id < p.pieces;
  const int64_t idc = live ? id : 0;  // (idle lanes walk piece 0 and store nothing: the butterflies need every lane)
  const int ppr = p.Kp >> 5;
  const int n = (int)(idc / ppr), rem = (int)(idc - (int64_t)n * ppr), sb = rem >> 2, kq = rem & 3;
  float f[4][8], mn[4], mx[4];
  bool has[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = 128 * sb + 32 * c;
    has[c] = k < p.K;  // (32 | K: a run lies inside K or in the padding)
    u32x4 v = {0u, 0u, 0u, 0u};
    if (has[c]) v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.w + (size_t)n * p.K + k + 8 * kq));
    unpack_bf16x8(v, f[c]);
    mn[c] = 0.f, mx[c] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) mn[c] = fminf(mn[c], f[c][j]), mx[c] = fmaxf(mx[c], f[c][j]);
  }
  auto join = [&](auto& v, auto op) {  // the runs of one group hold the group's value
    if (p.g >= 64) v[0] = v[1] = op(v[0], v[1]), v[2] = v[3] = op(v[2], v[3]);
    if (p.g == 128) v[0] = v[1] = v[2] = v[3] = op(v[0], v[2]);
  };
  join(mn, [](float a, float b) { return fminf(a, b); });
  join(mx, [](float a, float b) { return fmaxf(a, b); });
  const float eps = round_bf16(kWeightEps);
  uint32_t dw[4] = {0u, 0u, 0u, 0u};
  int sum[4], zw[4];
  float s[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int off = 1; off < 4; off <<= 1) mn[c] = fminf(mn[c], __shfl_xor(mn[c], off)), mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], off));
    float zp;
    da8w4_qparams(mn[c], mx[c], 15.f, eps, s[c], zp);
    zw[c] = (int)zp;
    const float inv = 1.0f / s[c];
    sum[c] = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = has[c] ? (int)fminf(fmaxf(rintf(f[c][j] * inv) + zp, 0.f), 15.f) : 0;
      sum[c] += q - (has[c] ? zw[c] : 0);
      dw[2 * (c & 1) + (j >> 2)] |= (uint32_t)q << (8 * (j & 3) + 4 * (c >> 1));
    }
  }
  join(sum, [](int a, int b) { return a + b; });
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int off = 1; off < 4; off <<= 1) sum[c] += __shfl_xor(sum[c], off);
  }
  if (!live) return;
  *reinterpret_cast<u32x4*>(p.packed + (size_t)id * 4) = u32x4{dw[0], dw[1], dw[2], dw[3]};
  if (kq != 0) return;
  const int rpg = p.g >> 5;  // runs a group
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (!has[c] || (c & (rpg - 1)) != 0) continue;
    const size_t at = (size_t)((128 * sb + 32 * c) / p.g) * p.N + n;
    p.sz[2 * at] = s[c];
    p.sz[2 * at + 1] = bits_to_f32(((uint32_t)sum[c] << 16) | (uint32_t)zw[c]);
    p.qzeros[at] = (int8_t)zw[c];
    p.comp[at] = (int16_t)sum[c];
  }
}

// ---- dequantize: a thread a piece ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRowThreads) void da8w4_dequantize_kernel(const uint32_t* packed, const float* sz, uint16_t* out, int64_t pieces,
                                                                        int N, int K, int Kp, int g) {
  const int64_t id = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  if (id >= pieces) return;
  const int ppr = Kp >> 5;
  const int n = (int)(id / ppr), rem = (int)(id - (int64_t)n * ppr), sb = rem >> 2, kq = rem & 3;
  const u32x4 v = *reinterpret_cast<const u32x4*>(packed + (size_t)id * 4);
  const uint32_t dw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = 128 * sb + 32 * c;
    if (k >= K) continue;
    const size_t at = (size_t)(k / g) * N + n;
    const float s = sz[2 * at];
    const float zw = (float)(int)(f32_to_bits(sz[2 * at + 1]) & 0xffffu);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = ((float)((dw[2 * (c & 1) + (j >> 2)] >> (8 * (j & 3) + 4 * (c >> 1))) & 15u) - zw) * s;
    *reinterpret_cast<u32x4*>(out + (size_t)n * K + k + 8 * kq) = pack_bf16x8(f);
  }
}

// ---- the activation cast: one workgroup a row, the second pass reads the row from cache; g / 8 adjacent lanes hold a group ---------------
struct Da8w4ActArgs {
  const uint16_t* x;  // bf16 [M][K]
  int8_t* q;          // [M][Kp], zero past K
  float* scale;       // [M]
  int32_t* zp;        // [M], the reference's zero-point (0 .. 255; 0 when symmetric)
  uint32_t* meta;     // [M][Gp]: (-sum_k a, -za') as two int16, zero past G
  int K, Kp, g, G, Gp, symmetric;
};

__global__ __launch_bounds__(kRowThreads) void da8w4_quantize_act_kernel(Da8w4ActArgs p) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const u32x4* xr = reinterpret_cast<const u32x4*>(p.x + row * p.K);
  const int nvec = p.K >> 3, nvecp = p.Kp >> 3;
  float mn = 0.f, mx = 0.f;
  for (int i = tid; i < nvec; i += kRowThreads) {
    float f[8];
    unpack_bf16x8(xr[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) mn = fminf(mn, f[j]), mx = fmaxf(mx, f[j]);
  }
  mx = block_max(mx, red);
  mn = -block_max(-mn, red);
  float s, zp, lo, hi;
  int shift;  // what the stored int8 code lacks of the reference's
  if (p.symmetric) {
    s = fmaxf(round_bf16(fmaxf(-mn, mx) / 127.0f), kActEps);
    zp = 0.f, lo = -127.f, hi = 127.f, shift = 0;
  } else {
    da8w4_qparams(mn, mx, 255.f, kActEps, s, zp);
    lo = 0.f, hi = 255.f, shift = 128;
  }
  const float inv = 1.0f / s;
  const int za = (int)zp - shift;
  const int lpg = p.g >> 3;
  for (int base = 0; base < nvecp; base += kRowThreads) {  // (the trip count is the workgroup's: the butterflies need every lane)
    const int i = base + tid;
    int sum = 0;
    u32x2 o = {0u, 0u};
    if (i < nvec) {
      float f[8];
      unpack_bf16x8(xr[i], f);
      uint32_t c[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int a = (int)fminf(fmaxf(rintf(f[j] * inv) + zp, lo), hi) - shift;
        sum += a;
        c[j] = (uint32_t)a & 0xffu;
      }
      o = u32x2{c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24), c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24)};
    }
    if (i < nvecp) *reinterpret_cast<u32x2*>(p.q + row * p.Kp + ((int64_t)i << 3)) = o;
    for (int off = 1; off < lpg; off <<= 1) sum += __shfl_xor(sum, off);
    if (i < nvec && (tid & (lpg - 1)) == 0) p.meta[row * p.Gp + i / lpg] = ((uint32_t)(-sum) & 0xffffu) | ((uint32_t)(-za) << 16);
  }
  if (tid < p.Gp - p.G) p.meta[row * p.Gp + p.G + tid] = 0u;
  if (tid == 0) {
    p.scale[row] = s;
    p.zp[row] = (int)zp;
  }
}

// ---- the linear -------------------------------------------------------------------------------------------------------------------------
struct Da8w4Args {
  const int8_t* a;       // [M][Kp]
  const uint32_t* w;     // [N][Kp / 8]
  const float* sz;       // [G][N][2]
  const uint32_t* ameta; // [M][Gp]
  const float* sa;       // [M]
  const uint16_t* bias;  // bf16 [N] or null
  uint16_t* out;         // bf16 [M][N]
  int M, N, Kp, G, Gp;
};

constexpr uint32_t kNibbles = 0x0f0f0f0fu;
template <int T>
__device__ __forceinline__ i32x4 da8w4_plane(u32x4 v) {
  if (T == 0) return i32x4{(int)(v.x & kNibbles), (int)(v.y & kNibbles), (int)(v.z & kNibbles), (int)(v.w & kNibbles)};
  return i32x4{(int)((v.x >> 4) & kNibbles), (int)((v.y >> 4) & kNibbles), (int)((v.z >> 4) & kNibbles), (int)((v.w >> 4) & kNibbles)};
}
__device__ __forceinline__ long da8w4_pair(int lo, int hi) { return (long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo); }

// Stream form.  grid (N / 16, m-tiles of 16), WAVES waves.  Wave w takes the 128-k steps w, w + WAVES, ...: the steps of one 2048-k chunk
// are in LDS together (rows kStreamRowStride apart: the 8-byte reads of 16 rows x 4 lane groups spread over the banks), and a wave keeps up
// to four weight requests in flight beyond the ones it works on.  The meeting buffer reuses the chunk's LDS.
constexpr int kStreamChunk = 2048;
constexpr int kStreamRowStride = kStreamChunk + 32;

template <int GS, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void da8w4_stream_kernel(Da8w4Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int SPC = 16 / WAVES, D = SPC < 4 ? SPC : 4, BPC = SPC / D;  // steps a wave and chunk, steps a batch, batches a chunk
  const int tid = threadIdx.x, lane = tid & 63, nl = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.y * 16, n0 = blockIdx.x * 16;
  const int rows = min(16, p.M - m0);
  const bool has_row = nl < rows;
  const int nsteps = p.Kp >> 7, nchunks = (nsteps + 15) >> 4;
  const uint32_t* wrow = p.w + (size_t)(n0 + nl) * (size_t)(p.Kp >> 3) + 4 * kq;  // (N % 32 == 0: every column of the tile exists)
  const uint32_t* am = p.ameta + (size_t)(m0 + (has_row ? nl : 0)) * p.Gp;
  const float* sz = p.sz + (size_t)(n0 + 4 * kq) * 2;

  auto issue = [&](u32x4 (&st)[D], int b) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int s = wave + (b * D + d) * WAVES;
      st[d] = u32x4{0u, 0u, 0u, 0u};
      if (s < nsteps) st[d] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow + (size_t)s * 16));
    }
    __builtin_amdgcn_sched_barrier(0);  // every request of the batch is out before anything waits
  };
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  auto fold = [&](int grp, i32x4 P) {
    if (grp >= p.G) return;  // (the padding of the last superblock: wave-uniform)
    const float* z = sz + (size_t)grp * p.N * 2;
    const f32x4 z0 = *reinterpret_cast<const f32x4*>(z), z1 = *reinterpret_cast<const f32x4*>(z + 4);
    const uint32_t ma = has_row ? am[grp] : 0u;
    acc.x = fmaf((float)da8w4_group_sum(f32_to_bits(z0.y), ma, P.x), z0.x, acc.x);
    acc.y = fmaf((float)da8w4_group_sum(f32_to_bits(z0.w), ma, P.y), z0.z, acc.y);
    acc.z = fmaf((float)da8w4_group_sum(f32_to_bits(z1.y), ma, P.z), z1.x, acc.z);
    acc.w = fmaf((float)da8w4_group_sum(f32_to_bits(z1.w), ma, P.w), z1.z, acc.w);
  };
  auto step = [&](u32x4 wp, int s) {
    const char* xa = smem + nl * kStreamRowStride + ((s & 15) << 7) + 8 * kq;
    i32x4 P = {0, 0, 0, 0};
    auto plane = [&](auto tt) {
      constexpr int T = decltype(tt)::value;
      const i32x4 wt = da8w4_plane<T>(wp);
      u32x2 lo = {0u, 0u}, hi = {0u, 0u};
      if (has_row) lo = *reinterpret_cast<const u32x2*>(xa + 64 * T), hi = *reinterpret_cast<const u32x2*>(xa + 64 * T + 32);
      if constexpr (GS >= 64) {
        P = __builtin_amdgcn_mfma_i32_16x16x64_i8(wt, i32x4{(int)lo.x, (int)lo.y, (int)hi.x, (int)hi.y}, P, 0, 0, 0);
        if (GS == 64 || T == 1) {
          fold(GS == 64 ? 2 * s + T : s, P);
          P = i32x4{0, 0, 0, 0};
        }
      } else {
        const i32x4 zero = {0, 0, 0, 0};
        fold(4 * s + 2 * T, __builtin_amdgcn_mfma_i32_16x16x32_i8(da8w4_pair(wt.x, wt.y), da8w4_pair((int)lo.x, (int)lo.y), zero, 0, 0, 0));
        fold(4 * s + 2 * T + 1, __builtin_amdgcn_mfma_i32_16x16x32_i8(da8w4_pair(wt.z, wt.w), da8w4_pair((int)hi.x, (int)hi.y), zero, 0, 0, 0));
      }
    };
    plane(std::integral_constant<int, 0>{});
    plane(std::integral_constant<int, 1>{});
  };

  u32x4 cur[D], nxt[D];
  issue(cur, 0);
  const int nbatches = nchunks * BPC;
  for (int b = 0; b < nbatches; ++b) {
    if (b % BPC == 0) {
      const int k0 = (b / BPC) * kStreamChunk;
      const int pieces = min(kStreamChunk, p.Kp - k0) >> 4;
      if (b != 0) lds_barrier();  // the previous chunk has been read
      for (int u = tid; u < rows * pieces; u += 64 * WAVES) {
        const int r = u / pieces, pc = u - r * pieces;
        *reinterpret_cast<u32x4*>(smem + r * kStreamRowStride + (pc << 4)) =
            *reinterpret_cast<const u32x4*>(p.a + (size_t)(m0 + r) * p.Kp + k0 + (pc << 4));
      }
      lds_barrier();
    }
    if (b + 1 < nbatches) issue(nxt, b + 1);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int s = wave + (b * D + d) * WAVES;
      if (s < nsteps) step(cur[d], s);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) cur[d] = nxt[d];
  }
  // the waves' K shares meet in wave order: lane (row nl, group kq) holds columns 4 kq .. + 3
  f32x4* red = reinterpret_cast<f32x4*>(smem);
  lds_barrier();  // the last chunk has been read
  red[wave * 64 + lane] = acc;
  lds_barrier();
  if (wave != 0 || !has_row) return;
  f32x4 c = red[lane];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) c += red[w * 64 + lane];
  const int m = m0 + nl, n = n0 + 4 * kq;
  const float sa = p.sa[m];
  const bool has_bias = p.bias != nullptr;
  uint16_t o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = da8w4_out(c[e], sa, has_bias, has_bias ? bf16_lo_to_f32(p.bias[n + e]) : 0.f);
  *reinterpret_cast<u32x2*>(p.out + (size_t)m * p.N + n) = u32x2{(uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16)};
}

// Tiled form.  grid (n-tiles of 64, m-tiles of 128), four waves as 2 x 2, a wave owns 64 rows x 32 columns = 4 x 2 MFMA tiles.  An LDS stage:
//   A  [128 rows][128 bytes]  the 16-byte piece c of row r at slot c ^ ((r >> 1) & 7)
//   W  [64 rows][64 bytes]    the packed piece kq of row r at slot kq ^ ((r >> 2) & 3)
//   Z  [4][64 columns][8 bytes]  scale_and_zero of the step's groups: 128 / g of the four slots are read, the others hold clamped duplicates
//                                (1.5 KiB of redundant DMA a step at g = 128, 1 KiB at g = 64: every wave issues the same six instructions)
//   Mt [128 rows][16 bytes]   act_meta of the aligned four groups around the step's
// Every wave issues six DMA instructions a step: four for A, one for W, one for Z (waves 0, 1) or Mt (waves 2, 3).
constexpr int kTileM = 128, kTileN = 64, kTileStages = 3;
constexpr int kTileA = 0, kTileW = 16384, kTileZ = 20480, kTileMt = 22528, kTileStageBytes = 24576;
constexpr int kTileDmaPerStep = 6;
constexpr int kTileLdsBytes = kTileStages * kTileStageBytes;

template <int GS>
__global__ __launch_bounds__(256) void da8w4_tile_kernel(Da8w4Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int GPS = 128 / GS;  // groups a step
  const int tid = threadIdx.x, lane = tid & 63, ml = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * kTileM, n0 = blockIdx.x * kTileN;
  const int T = p.Kp >> 7;
  const uint32_t lds0 = lds_offset(smem);

  // this lane's DMA sources; rows and columns past the edge read the last valid one (never stored)
  uint32_t av[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 32 * wave + 8 * i + (lane >> 3);  // (r >> 1) & 7 = 4 (i & 1) + (lane >> 4)
    av[i] = (uint32_t)min(r, p.M - 1 - m0) * (uint32_t)p.Kp + (uint32_t)(((lane & 7) ^ (4 * (i & 1) + (lane >> 4))) << 4);
  }
  const uint32_t wv = (uint32_t)min(16 * wave + (lane >> 2), p.N - 1 - n0) * (uint32_t)(p.Kp >> 1) + (uint32_t)(((lane & 3) ^ (lane >> 4)) << 4);
  const int zsel = min(2 * wave + (lane >> 5), GPS - 1);                   // waves 0, 1: the group of the step this lane fetches
  const uint32_t zcol = (uint32_t)(n0 + min(2 * (lane & 31), p.N - n0 - 2));
  const uint32_t mrow = (uint32_t)min(64 * (wave & 1) + lane, p.M - 1 - m0) * (uint32_t)p.Gp * 4u;  // waves 2, 3
  const char* abase = reinterpret_cast<const char*>(p.a) + (size_t)m0 * p.Kp;
  const char* wbase = reinterpret_cast<const char*>(p.w) + (size_t)n0 * (size_t)(p.Kp >> 1);
  const char* mbase = reinterpret_cast<const char*>(p.ameta) + (size_t)m0 * p.Gp * 4;
  auto issue = [&](int t) {
    const uint32_t st = lds0 + (uint32_t)(t % kTileStages) * kTileStageBytes;
    dma_b128_x4(abase + (size_t)t * 128, av[0], av[1], av[2], av[3], st + kTileA + wave * 4096);
    dma_b128_s(wbase + (size_t)t * 64, wv, st + kTileW + wave * 1024);
    if (wave < 2) {
      const uint32_t grp = (uint32_t)min(t * GPS + zsel, p.G - 1);
      dma_b128_s(p.sz, (grp * (uint32_t)p.N + zcol) * 8u, st + kTileZ + wave * 1024);
    } else {
      dma_b128_s(mbase, mrow + (uint32_t)(((t * GPS) >> 2) << 4), st + kTileMt + (wave & 1) * 1024);
    }
  };

  i32x4 P[4][2];
  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) P[i][j] = i32x4{0, 0, 0, 0}, acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue(0);
  if (T > 1) issue(1);
  for (int t = 0; t < T; ++t) {
    // step t has landed for this wave (the DMAs return in order); past the barrier for all of them, and stage (t + 2) % 3 = (t - 1) % 3 is read out
    if (t + 1 < T) wait_vmcnt<kTileDmaPerStep>();
    else wait_vmcnt<0>();
    lds_barrier();
    if (t + 2 < T) issue(t + 2);
    const char* S = smem + (t % kTileStages) * kTileStageBytes;
    // group `gsel` of the step is complete in P: fold it into acc
    auto fold = [&](int gsel) {
      const int grp = t * GPS + gsel;
      if (grp >= p.G) return;  // (the padding of the last superblock)
      uint32_t ma[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ma[i] = *reinterpret_cast<const uint32_t*>(S + kTileMt + (wm * 64 + i * 16 + ml) * 16 + (grp & 3) * 4);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const char* z = S + kTileZ + gsel * 512 + (wn * 32 + j * 16 + 4 * kq) * 8;
        const f32x4 z0 = *reinterpret_cast<const f32x4*>(z), z1 = *reinterpret_cast<const f32x4*>(z + 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[i][j].x = fmaf((float)da8w4_group_sum(f32_to_bits(z0.y), ma[i], P[i][j].x), z0.x, acc[i][j].x);
          acc[i][j].y = fmaf((float)da8w4_group_sum(f32_to_bits(z0.w), ma[i], P[i][j].y), z0.z, acc[i][j].y);
          acc[i][j].z = fmaf((float)da8w4_group_sum(f32_to_bits(z1.y), ma[i], P[i][j].z), z1.x, acc[i][j].z);
          acc[i][j].w = fmaf((float)da8w4_group_sum(f32_to_bits(z1.w), ma[i], P[i][j].w), z1.z, acc[i][j].w);
          P[i][j] = i32x4{0, 0, 0, 0};
        }
      }
    };
    u32x4 wp[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = wn * 32 + j * 16 + ml;
      wp[j] = *reinterpret_cast<const u32x4*>(S + kTileW + r * 64 + ((kq ^ ((r >> 2) & 3)) << 4));
    }
    auto plane = [&](auto tt) {
      constexpr int TT = decltype(tt)::value;
      const i32x4 wt[2] = {da8w4_plane<TT>(wp[0]), da8w4_plane<TT>(wp[1])};
      // the 8-byte run 64 TT + 32 h + 8 kq of row r: piece 4 TT + 2 h + (kq >> 1), its half kq & 1
      auto run = [&](int r, int h) {
        return *reinterpret_cast<const u32x2*>(S + kTileA + r * 128 + (((4 * TT + 2 * h + (kq >> 1)) ^ ((r >> 1) & 7)) << 4) + 8 * (kq & 1));
      };
      if constexpr (GS >= 64) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = wm * 64 + i * 16 + ml;
          const u32x2 lo = run(r, 0), hi = run(r, 1);
          const i32x4 aop = {(int)lo.x, (int)lo.y, (int)hi.x, (int)hi.y};
#pragma unroll
          for (int j = 0; j < 2; ++j) P[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wt[j], aop, P[i][j], 0, 0, 0);
        }
        if (GS == 64 || TT == 1) fold(GS == 64 ? TT : 0);
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const u32x2 a8 = run(wm * 64 + i * 16 + ml, h);
#pragma unroll
            for (int j = 0; j < 2; ++j)
              P[i][j] = __builtin_amdgcn_mfma_i32_16x16x32_i8(h == 0 ? da8w4_pair(wt[j].x, wt[j].y) : da8w4_pair(wt[j].z, wt[j].w),
                                                              da8w4_pair((int)a8.x, (int)a8.y), P[i][j], 0, 0, 0);
          }
          fold(2 * TT + h);
        }
      }
    };
    plane(std::integral_constant<int, 0>{});
    plane(std::integral_constant<int, 1>{});
  }

  // W was the MFMA's A: lane (row ml of the m-tile, group kq) holds columns 4 kq .. + 3 of the n-tile
  const bool has_bias = p.bias != nullptr;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + ml;
    if (m >= p.M) continue;
    const float sa = p.sa[m];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 32 + j * 16 + kq * 4;
      if (n >= p.N) continue;  // (4 | N: the four columns exist together)
      uint16_t o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = da8w4_out(acc[i][j][e], sa, has_bias, has_bias ? bf16_lo_to_f32(p.bias[n + e]) : 0.f);
      *reinterpret_cast<u32x2*>(p.out + (size_t)m * p.N + n) =
          u32x2{(uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16)};
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
inline int64_t padded_k(int64_t K) { return (K + 127) / 128 * 128; }
inline int64_t padded_groups(int64_t K, int64_t g) { return (K / g + 3) / 4 * 4; }

int da8w4_check_group(const char* fn, int64_t K, int64_t g) {
  AO_REQUIRE(g == 32 || g == 64 || g == 128, "%s: group_size=%lld must be 32, 64 or 128", fn, (long long)g);
  AO_REQUIRE(K > 0 && K % g == 0, "%s: K=%lld must be a positive multiple of group_size=%lld", fn, (long long)K, (long long)g);
  AO_REQUIRE(K <= (1ll << 24), "%s: K=%lld too large (K <= 2^24)", fn, (long long)K);
  return AO_OK;
}

int da8w4_check_weight(const char* fn, int64_t N, int64_t K, int64_t g) {
  if (int rc = da8w4_check_group(fn, K, g)) return rc;
  AO_REQUIRE(N > 0 && N % 32 == 0, "%s: N=%lld must be a positive multiple of 32", fn, (long long)N);
  AO_REQUIRE(N * padded_k(K) < (1ll << 32), "%s: N=%lld x K=%lld too large (the packed weight must stay below 2^31 bytes)", fn, (long long)N,
             (long long)K);
  return AO_OK;
}

int da8w4_check_shape(const char* fn, int64_t M, int64_t N, int64_t K, int64_t g) {
  if (int rc = da8w4_check_weight(fn, N, K, g)) return rc;
  AO_REQUIRE(M >= 0, "%s: bad shape M=%lld", fn, (long long)M);
  AO_REQUIRE(M * padded_k(K) < (1ll << 31) && M * N < (1ll << 40), "%s: M=%lld too large for N=%lld K=%lld (the activation codes must stay below 2^31 bytes)",
             fn, (long long)M, (long long)N, (long long)K);
  return AO_OK;
}

// kernel 1: da8w4_stream_kernel (one m-tile a workgroup, more rows add grid rows), 2: da8w4_tile_kernel (128 x 64 tiles)
TwoFormRoute da8w4_route(int64_t M, int64_t N, int64_t K, int64_t g) {
  if (da8w4_check_shape("ao_da8w4_linear_route", M, N, K, g) != AO_OK) return TwoFormRoute{};
  const int form = g_form != 0 ? g_form : (M <= kStreamMaxRows ? 1 : 2);
  TwoFormRoute r;
  if (form == 1) {
    r = stream_form_plan(std::min<int64_t>(M, 16), N, K);
    r.grid_y = (int)std::max<int64_t>(1, (M + 15) / 16);
  } else {
    r = tiled_form_plan(M, N, kTileN);
    r.mt = kTileM / 16;
    r.tile_m = kTileM;
    r.grid_y = (int)((M + kTileM - 1) / kTileM);
  }
  if (r.grid_y > 65535) r.kernel = 0;
  return r;
}

template <int GS>
int launch_linear(const TwoFormRoute& r, const Da8w4Args& a, hipStream_t st) {
  if (r.kernel == 2)
    return launch_tile_form(da8w4_tile_kernel<GS>, "da8w4_tile_kernel launch", r, a, st, kTileLdsBytes, "da8w4_tile_kernel dynamic LDS");
  auto go = [&](auto waves) {
    constexpr int W = decltype(waves)::value;
    const size_t smem = std::max<size_t>((size_t)W * 1024, (size_t)std::min(a.M, 16) * kStreamRowStride);  // at most 33280 bytes
    ao::launch(da8w4_stream_kernel<GS, W>, dim3(r.grid_x, r.grid_y), dim3(64 * W), smem, st, a);
  };
  switch (r.waves) {
    case 1: go(std::integral_constant<int, 1>{}); break;
    case 2: go(std::integral_constant<int, 2>{}); break;
    case 4: go(std::integral_constant<int, 4>{}); break;
    case 8: go(std::integral_constant<int, 8>{}); break;
    case 16: go(std::integral_constant<int, 16>{}); break;
    default: set_error("da8w4_stream_kernel: no instantiation for %d waves", r.waves); return AO_ERR_INVALID_ARGUMENT;
  }
  AO_LAUNCH_CHECK("da8w4_stream_kernel launch");
  return AO_OK;
}

int piece_grid(int64_t pieces) { return (int)((pieces + kRowThreads - 1) / kRowThreads); }

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_da8w4_quantize_weight(const uint16_t* w, uint32_t* packed, float* scale_and_zero, int8_t* qzeros, int16_t* compensation, int64_t N,
                                        int64_t K, int64_t group_size, void* stream) {
  if (int rc = da8w4_check_weight(__func__, N, K, group_size)) return rc;
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(packed);
  AO_REQUIRE_PTR(scale_and_zero);
  AO_REQUIRE_PTR(qzeros);
  AO_REQUIRE_PTR(compensation);
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(packed, 16) && aligned_to(scale_and_zero, 16) && aligned_to(compensation, 2),
             "%s: w, packed and scale_and_zero must be 16-byte aligned, compensation 2-byte", __func__);
  const int64_t Kp = padded_k(K), pieces = N * (Kp / 32);
  const Da8w4WeightArgs a{w, packed, scale_and_zero, qzeros, compensation, pieces, (int)N, (int)K, (int)Kp, (int)group_size};
  ao::launch(da8w4_quantize_weight_kernel, dim3(piece_grid(pieces)), dim3(kRowThreads), 0, (hipStream_t)stream, a);
  AO_LAUNCH_CHECK("da8w4_quantize_weight_kernel launch");
  return AO_OK;
}

extern "C" int ao_da8w4_dequantize(const uint32_t* packed, const float* scale_and_zero, uint16_t* out, int64_t N, int64_t K, int64_t group_size,
                                   void* stream) {
  if (int rc = da8w4_check_weight(__func__, N, K, group_size)) return rc;
  AO_REQUIRE_PTR(packed);
  AO_REQUIRE_PTR(scale_and_zero);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(packed, 16) && aligned_to(scale_and_zero, 4) && aligned_to(out, 16), "%s: packed and out must be 16-byte aligned, scale_and_zero 4-byte",
             __func__);
  const int64_t Kp = padded_k(K), pieces = N * (Kp / 32);
  ao::launch(da8w4_dequantize_kernel, dim3(piece_grid(pieces)), dim3(kRowThreads), 0, (hipStream_t)stream, packed, scale_and_zero, out, pieces, (int)N,
             (int)K, (int)Kp, (int)group_size);
  AO_LAUNCH_CHECK("da8w4_dequantize_kernel launch");
  return AO_OK;
}

extern "C" int ao_da8w4_quantize_act(const uint16_t* x, int8_t* q, float* scale, int32_t* zero_point, uint32_t* act_meta, int64_t M, int64_t K,
                                     int64_t group_size, int symmetric, void* stream) {
  if (int rc = da8w4_check_group(__func__, K, group_size)) return rc;
  AO_REQUIRE(M >= 0 && M * padded_k(K) < (1ll << 31), "%s: M=%lld too large for K=%lld (the codes must stay below 2^31 bytes)", __func__, (long long)M,
             (long long)K);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(scale);
  AO_REQUIRE_PTR(zero_point);
  AO_REQUIRE_PTR(act_meta);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(q, 16) && aligned_to(act_meta, 16) && aligned_to(scale, 4) && aligned_to(zero_point, 4),
             "%s: x, q and act_meta must be 16-byte aligned, scale and zero_point 4-byte", __func__);
  const int64_t G = K / group_size;
  const Da8w4ActArgs a{x, q, scale, zero_point, act_meta, (int)K, (int)padded_k(K), (int)group_size, (int)G, (int)padded_groups(K, group_size),
                       symmetric != 0 ? 1 : 0};
  ao::launch(da8w4_quantize_act_kernel, dim3((unsigned)M), dim3(kRowThreads), 0, (hipStream_t)stream, a);
  AO_LAUNCH_CHECK("da8w4_quantize_act_kernel launch");
  return AO_OK;
}

extern "C" int ao_da8w4_linear_fits(int64_t M, int64_t N, int64_t K, int64_t group_size) {
  return da8w4_check_shape(__func__, M, N, K, group_size) == AO_OK ? 1 : 0;
}

extern "C" int ao_da8w4_linear_route(int64_t M, int64_t N, int64_t K, int64_t group_size, int32_t* out, int cap) {
  return route_export(__func__, da8w4_route(M, N, K, group_size), out, cap);
}

extern "C" const char* ao_da8w4_linear_kernel_name(int64_t M, int64_t N, int64_t K, int64_t group_size) {
  return route_kernel_name(da8w4_route(M, N, K, group_size), "da8w4_stream_kernel", "da8w4_tile_kernel");
}

extern "C" int ao_da8w4_linear_set_form(int form) { return set_forced_form(__func__, form, g_form); }

extern "C" int ao_da8w4_linear(const int8_t* q, const uint32_t* packed, const float* scale_and_zero, const uint32_t* act_meta, const float* act_scale,
                               const uint16_t* bias, uint16_t* out, int64_t M, int64_t N, int64_t K, int64_t group_size, void* stream) {
  if (int rc = da8w4_check_shape(__func__, M, N, K, group_size)) return rc;
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(packed);
  AO_REQUIRE_PTR(scale_and_zero);
  AO_REQUIRE_PTR(act_meta);
  AO_REQUIRE_PTR(act_scale);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(q, 16) && aligned_to(packed, 16) && aligned_to(scale_and_zero, 16) && aligned_to(act_meta, 16) && aligned_to(out, 8) &&
                 aligned_to(act_scale, 4) && aligned_to(bias, 2),
             "%s: q, packed, scale_and_zero and act_meta must be 16-byte aligned, out 8-byte, act_scale 4-byte, bias 2-byte", __func__);
  const TwoFormRoute r = da8w4_route(M, N, K, group_size);
  AO_REQUIRE(r.kernel != 0, "%s: no route for M=%lld N=%lld K=%lld (more than 65535 grid rows)", __func__, (long long)M, (long long)N, (long long)K);
  const Da8w4Args a{q, packed, scale_and_zero, act_meta, act_scale, bias, out, (int)M, (int)N, (int)padded_k(K), (int)(K / group_size),
                    (int)padded_groups(K, group_size)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (group_size == 32) return launch_linear<32>(r, a, st);
  if (group_size == 64) return launch_linear<64>(r, a, st);
  return launch_linear<128>(r, a, st);
}
