// FP8 attention for gfx950: the per-head e4m3 cast of Q / K / V and a flash-attention forward on the fp8 matrix pipe.
//
// Reference (torchao 0.19.0 snapshot): prototype/attention/quantization/triton_qkv_quantization.py:102-166, 240, 264-460 (the cast: three
// amax launches, three reductions, three casts) and shared_utils/attention.py:37-96 (_fp8_sdpa: the cast, then the FA3 kernel the
// reference can only reach on Hopper).  Here: two launches for the cast, one for the attention.
//
//   A  fp8_attn_amax_kernel   state[t][b][hkv] = max |x|  over the rows (and, for Q, the Hq / Hkv query heads) of one kv head   t = q, k, v
//   B  fp8_attn_cast_kernel   scale = amax > 1e-12 ? 448 / amax : 1;  descale = amax > 1e-12 ? amax / 448 : 1   (IEEE fp32 divisions)
//                             code  = e4m3fn_rne(clamp(f32(x) * scale, +-448))        contiguous [B][H][S][D]
//   C  fp8_attn_fwd_kernel<D, CAUSAL>
//        out[b][h][i][:] = softmax_j(scale dq dk sum_d Qc[i][d] Kc[j][d]) dv Vc[j][:]         fp32 accumulation and softmax, one rounding at the store
//
// A and B take any strides on B / H / S (D contiguous): the [B, S, H, D].transpose(1, 2) view is read in place.  A folds with atomicMax on
// the bit pattern of non-negative floats (smoothquant_kernels.hip: exact, order-independent) into a zeroed state the caller supplies.
//
// C.  One workgroup = one 128-row query tile of one (batch, query head): 4 waves x 32 query rows (two 16-wide column tiles of the MFMA).
//   * Q fragments (B operand of the first product) stay in registers: lane (i = lane & 15, g = lane >> 4) holds Q[i][32 s + 8 g ..+7].
//   * K and V walk in 64-row tiles through two LDS stages of 2 x 64 x D bytes; one workgroup barrier per tile.
//     K: global_load_lds_dwordx4 (lds_dma.h).  The DMA writes LDS in lane order, so the swizzle is in the SOURCE address: LDS chunk
//     (row R, position p) holds the row's 16-byte chunk p ^ key(R), and the 16 rows a fragment read touches fall on 16 distinct 16-byte
//     bank groups (key: see kkey).
//     V: 4 x 4 byte blocks through registers, transposed by v_perm_b32 (8 per block), stored as Vt[d][kv] so that the second product's
//     A operand is one 8-byte read of kv-contiguous bytes; 8-byte units of a row are XOR-swizzled by ((d >> 2) & 3) << 1.
//   * S^T = K Q^T with K as the A operand.  Row m of S-tile (u, half) is kv row 32 u + 8 (m >> 2) + 4 half + (m & 3), so lane group g's eight
//     accumulator registers of the two tiles of a pair u are the kv indices 32 u + 8 g ..+7 of ONE query column: exactly the B operand
//     of O^T += Vt P^T.  P never crosses lanes.
//   * Online softmax in base 2 on t = s * (scale dq dk log2 e); the running maximum is shared by the 4 lane groups of a column (two
//     ds_bpermute per tile and column tile), the running sum stays per lane until the epilogue.
//   * P is cast as e4m3(256 p) (p <= 1: the subnormal step falls at 2^-17 of the row maximum); the sum is taken from the fp32 values before
//     the cast and carries the same 256, so the epilogue's dv / l removes it.
//   * CAUSAL: query tiles heaviest first, KV tiles wholly above the diagonal never loaded, a wave skips the tiles above its own 32 rows.
// Rows past Sq / Skv are read clamped to the last row, masked to -inf (p = 0 exactly) and never stored.
#include <algorithm>

#include "common.h"
#include "lds_dma.h"
#include "quant_math.h"

namespace ao {
namespace {

typedef long i64_t;
typedef uint16_t u16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int kCastThreads = kRowThreads;
constexpr int kCastRows = 128;  // rows of one head a cast workgroup owns
constexpr int kQTile = 128, kKvTile = 64, kAttnThreads = 256;

// ---- A / B: the cast ----------------------------------------------------------------------------------------------------------------------------
struct AttnCastTensor {
  const uint16_t* x;
  uint8_t* codes;
  int64_t sb, sh, ss;  // element strides of batch, head, row
  int S, H;
};
struct AttnCastArgs {
  AttnCastTensor t[3];  // q, k, v
  int B, Hkv, groups, D;
};

// which tensor, batch, head and kv head workgroup column `hx` of the cast grid belongs to: [B Hq | B Hkv | B Hkv]
struct AttnCastWhere { int t, b, h, slot; };
__device__ __forceinline__ AttnCastWhere attn_cast_where(const AttnCastArgs& a, int hx) {
  const int nq = a.B * a.Hkv * a.groups, nkv = a.B * a.Hkv;
  AttnCastWhere w;
  if (hx < nq) { w.t = 0; w.b = hx / (a.Hkv * a.groups); w.h = hx % (a.Hkv * a.groups); w.slot = w.b * a.Hkv + w.h / a.groups; }
  else { hx -= nq; w.t = 1 + hx / nkv; hx %= nkv; w.b = hx / a.Hkv; w.h = hx % a.Hkv; w.slot = (w.t * a.B + w.b) * a.Hkv + w.h; }
  return w;
}
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2_t, a), __builtin_bit_cast(u16x2_t, b)));
}
template <bool F16>
__device__ __forceinline__ float half_to_f32(uint32_t bits16) {
  if constexpr (F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
  else return bits_to_f32(bits16 << 16);
}

template <bool F16>
__global__ __launch_bounds__(kCastThreads) void fp8_attn_amax_kernel(AttnCastArgs a, uint32_t* __restrict__ state) {
  __shared__ float red[4];
  const AttnCastWhere w = attn_cast_where(a, blockIdx.x);
  const AttnCastTensor& T = a.t[w.t];
  const int s0 = blockIdx.y * kCastRows;
  if (s0 >= T.S) return;
  const int vd = a.D >> 3, n = min(kCastRows, T.S - s0) * vd;
  const uint16_t* base = T.x + w.b * T.sb + w.h * T.sh;
  uint32_t m0 = 0u, m1 = 0u, m2 = 0u, m3 = 0u;  // running packed maxima of |x| as 15-bit patterns: non-negative bf16 and fp16 both order as integers
  for (int idx = threadIdx.x; idx < n; idx += kCastThreads) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(base + (int64_t)(s0 + idx / vd) * T.ss + (idx % vd) * 8);
    m0 = pk_max_u16(m0, v.x & 0x7fff7fffu);
    m1 = pk_max_u16(m1, v.y & 0x7fff7fffu);
    m2 = pk_max_u16(m2, v.z & 0x7fff7fffu);
    m3 = pk_max_u16(m3, v.w & 0x7fff7fffu);
  }
  const uint32_t m01 = pk_max_u16(m0, m1), m23 = pk_max_u16(m2, m3), m4 = pk_max_u16(m01, m23);
  const uint32_t top = (m4 & 0xffffu) > (m4 >> 16) ? (m4 & 0xffffu) : (m4 >> 16);
  const float f = block_max(half_to_f32<F16>(top), red);
  if (threadIdx.x == 0 && f != 0.f) atomicMax(state + w.slot, f32_to_bits(f));
}

template <bool F16>
__global__ __launch_bounds__(kCastThreads) void fp8_attn_cast_kernel(AttnCastArgs a, const float* __restrict__ state, float* __restrict__ descale) {
  const AttnCastWhere w = attn_cast_where(a, blockIdx.x);
  const AttnCastTensor& T = a.t[w.t];
  const int s0 = blockIdx.y * kCastRows;
  if (s0 >= T.S) return;
  const float amax = state[w.slot];
  const float scale = amax > 1e-12f ? 448.0f / amax : 1.0f;
  if (s0 == 0 && threadIdx.x == 0 && (w.t != 0 || w.h % a.groups == 0)) descale[w.slot] = amax > 1e-12f ? amax / 448.0f : 1.0f;
  const int vd = a.D >> 3, n = min(kCastRows, T.S - s0) * vd;
  const uint16_t* base = T.x + w.b * T.sb + w.h * T.sh;
  uint8_t* obase = T.codes + ((int64_t)(w.b * T.H + w.h) * T.S + s0) * a.D;
  for (int idx = threadIdx.x; idx < n; idx += kCastThreads) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(base + (int64_t)(s0 + idx / vd) * T.ss + (idx % vd) * 8);
    const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
    float f[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[2 * j] = fminf(fmaxf(half_to_f32<F16>(wd[j] & 0xffffu) * scale, -448.f), 448.f);
      f[2 * j + 1] = fminf(fmaxf(half_to_f32<F16>(wd[j] >> 16) * scale, -448.f), 448.f);
    }
    *reinterpret_cast<u32x2*>(obase + (int64_t)idx * 8) = u32x2{cvt4_e4m3(f[0], f[1], f[2], f[3]), cvt4_e4m3(f[4], f[5], f[6], f[7])};
  }
}

// ---- C: the attention forward --------------------------------------------------------------------------------------------------------------------
// swizzle key of K row R: the 16 rows of one fragment read (8 a + b + 4 half, a, b = 0..3) land on 16 distinct 16-byte bank groups
template <int D>
__device__ __forceinline__ int kkey(int R) {
  if constexpr (D == 128) return ((R >> 3) & 3) * 2 + ((R >> 1) & 1);  // bank group = (R & 1) * 8 + (chunk ^ key)
  else return (R >> 3) & 3;                                             // bank group = (R & 3) * 4 + (chunk ^ key)
}
// byte offset in a Vt stage of the 8-byte unit e (kv 8 e ..+7) of row d
__device__ __forceinline__ int vt_unit(int d, int e) { return d * kKvTile + ((e ^ (((d >> 2) & 3) << 1)) << 3); }

__device__ __forceinline__ float shfl_xor_f(float v, int mask) { return __shfl_xor(v, mask); }

template <int D, bool CAUSAL>
__global__ __launch_bounds__(kAttnThreads) void fp8_attn_fwd_kernel(const uint8_t* __restrict__ q8, const uint8_t* __restrict__ k8,
                                                                    const uint8_t* __restrict__ v8, const float* __restrict__ dq,
                                                                    const float* __restrict__ dk, const float* __restrict__ dv,
                                                                    uint16_t* __restrict__ out, int out_f16, int Hq, int Hkv, int Sq, int Skv,
                                                                    int nqt, float scale_log2e) {
  constexpr int STAGE = kKvTile * D;  // bytes of one K or Vt stage
  constexpr int CPR = D / 16;         // 16-byte chunks per K row
  constexpr int KDMA = STAGE / 4096;  // DMA instructions per wave and K tile (1 KiB each)
  constexpr int DQ = D / 4;           // 4-byte columns of a V row
  constexpr int NB = 16 * DQ / kAttnThreads;  // 4 x 4 blocks of a V tile per thread
  constexpr int DS = D / 32, DT = D / 16;
  __shared__ __attribute__((aligned(16))) uint8_t ks[2][STAGE];
  __shared__ __attribute__((aligned(16))) uint8_t vs[2][STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n16 = lane & 15, g = lane >> 4;
  const int qt = CAUSAL ? nqt - 1 - (int)blockIdx.x : (int)blockIdx.x;  // heaviest query tiles first
  const int h = blockIdx.y, b = blockIdx.z;
  const int hkv = h / (Hq / Hkv);
  const int q0 = qt * kQTile, qw = q0 + wave * 32;
  const bool wave_active = qw < Sq;
  const float c = scale_log2e * dq[b * Hkv + hkv] * dk[b * Hkv + hkv];
  const uint8_t* qb = q8 + (int64_t)(b * Hq + h) * Sq * D;
  const uint8_t* kb = k8 + (int64_t)(b * Hkv + hkv) * Skv * D;
  const uint8_t* vb = v8 + (int64_t)(b * Hkv + hkv) * Skv * D;

  i64_t qf[2][DS];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int row = min(qw + 16 * it + n16, Sq - 1);
#pragma unroll
    for (int s = 0; s < DS; ++s) qf[it][s] = *reinterpret_cast<const i64_t*>(qb + (int64_t)row * D + 32 * s + 8 * g);
  }

  int nkv = (Skv + kKvTile - 1) / kKvTile;
  if (CAUSAL) nkv = min(nkv, min(q0 + kQTile - 1, Sq - 1) / kKvTile + 1);

  const uint32_t ks_lds = lds_offset(&ks[0][0]);
  auto issue_k = [&](int t, int stage) {
#pragma unroll
    for (int n = 0; n < KDMA; ++n) {
      const int P = n * kAttnThreads + tid, R = P / CPR, p = P % CPR;
      const uint32_t row = (uint32_t)min(t * kKvTile + R, Skv - 1);
      dma_b128_s(kb, row * D + ((p ^ kkey<D>(R)) << 4), ks_lds + stage * STAGE + n * 4096 + wave * 1024);
    }
  };
  uint32_t vw[NB][4];
  const int vdq = tid % DQ;
  auto load_v = [&](int t) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int kvq = tid / DQ + n * (kAttnThreads / DQ);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t row = (uint32_t)min(t * kKvTile + 4 * kvq + r, Skv - 1);
        vw[n][r] = *reinterpret_cast<const uint32_t*>(vb + (size_t)row * D + 4 * vdq);
      }
    }
  };
  auto store_v = [&](int stage) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int kvq = tid / DQ + n * (kAttnThreads / DQ);
      // 4 x 4 byte transpose: rows kv 4 kvq ..+3, columns d 4 vdq ..+3
      const uint32_t lo01 = __builtin_amdgcn_perm(vw[n][1], vw[n][0], 0x05010400u), hi01 = __builtin_amdgcn_perm(vw[n][1], vw[n][0], 0x07030602u);
      const uint32_t lo23 = __builtin_amdgcn_perm(vw[n][3], vw[n][2], 0x05010400u), hi23 = __builtin_amdgcn_perm(vw[n][3], vw[n][2], 0x07030602u);
      const uint32_t o[4] = {__builtin_amdgcn_perm(lo23, lo01, 0x05040100u), __builtin_amdgcn_perm(lo23, lo01, 0x07060302u),
                             __builtin_amdgcn_perm(hi23, hi01, 0x05040100u), __builtin_amdgcn_perm(hi23, hi01, 0x07060302u)};
#pragma unroll
      for (int dd = 0; dd < 4; ++dd)
        *reinterpret_cast<uint32_t*>(&vs[stage][vt_unit(4 * vdq + dd, kvq >> 1) + (kvq & 1) * 4]) = o[dd];
    }
  };

  f32x4 o[DT][2];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt][0] = o[dt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_i[2] = {-INFINITY, -INFINITY}, l_i[2] = {0.f, 0.f};

  issue_k(0, 0);
  load_v(0);
  for (int t = 0; t < nkv; ++t) {
    const int stage = t & 1, kv0 = t * kKvTile;
    store_v(stage);
    wait_vmcnt<0>();  // this tile's K has landed
    __syncthreads();  // ... and every wave has left the stage the next requests overwrite
    if (t + 1 < nkv) {
      issue_k(t + 1, stage ^ 1);
      load_v(t + 1);
    }
    if (!wave_active || (CAUSAL && kv0 > qw + 31)) continue;  // (wave-uniform; the barrier above is the loop's only one)

    f32x4 s[2][4];
#pragma unroll
    for (int st = 0; st < 4; ++st) s[0][st] = s[1][st] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) {
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int R = 32 * (st >> 1) + 8 * (n16 >> 2) + 4 * (st & 1) + (n16 & 3);
        const i64_t a = *reinterpret_cast<const i64_t*>(&ks[stage][R * D + (((2 * ds + (g >> 1)) ^ kkey<D>(R)) << 4) + (g & 1) * 8]);
        s[0][st] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, qf[0][ds], s[0][st], 0, 0, 0);
        s[1][st] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, qf[1][ds], s[1][st], 0, 0, 0);
      }
    }
    const bool mask = kv0 + kKvTile > Skv || (CAUSAL && kv0 + kKvTile - 1 > qw);
    i64_t pb[2][2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i_row = qw + 16 * it + n16;
      float mx = -INFINITY;
#pragma unroll
      for (int st = 0; st < 4; ++st) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kv = kv0 + 32 * (st >> 1) + 8 * g + 4 * (st & 1) + r;
          float tv = s[it][st][r] * c;
          if (mask && (kv >= Skv || (CAUSAL && kv > i_row))) tv = -INFINITY;
          s[it][st][r] = tv;
          mx = fmaxf(mx, tv);
        }
      }
      mx = fmaxf(mx, shfl_xor_f(mx, 16));
      mx = fmaxf(mx, shfl_xor_f(mx, 32));
      const float m_new = fmaxf(m_i[it], mx);  // finite from the first tile on: key 0 is visible to every row
      const float alpha = __builtin_amdgcn_exp2f(m_i[it] - m_new);
      m_i[it] = m_new;
      const float mb = m_new - 8.0f;  // p256 = 256 p
      float sum = 0.f;
#pragma unroll
      for (int st = 0; st < 4; ++st) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(s[it][st][r] - mb);
          s[it][st][r] = p;
          sum += p;
        }
      }
      l_i[it] = l_i[it] * alpha + sum;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const uint32_t lo = cvt4_e4m3(s[it][2 * u][0], s[it][2 * u][1], s[it][2 * u][2], s[it][2 * u][3]);
        const uint32_t hi = cvt4_e4m3(s[it][2 * u + 1][0], s[it][2 * u + 1][1], s[it][2 * u + 1][2], s[it][2 * u + 1][3]);
        pb[it][u] = (i64_t)(((unsigned long)hi << 32) | lo);
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[dt][it] *= alpha;
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const i64_t a = *reinterpret_cast<const i64_t*>(&vs[stage][vt_unit(16 * dt + n16, 4 * u + g)]);
        o[dt][0] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, pb[0][u], o[dt][0], 0, 0, 0);
        o[dt][1] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, pb[1][u], o[dt][1], 0, 0, 0);
      }
    }
  }

  const float dvh = dv[b * Hkv + hkv];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    float l = l_i[it];
    l += shfl_xor_f(l, 16);
    l += shfl_xor_f(l, 32);
    const int i_row = qw + 16 * it + n16;
    if (!wave_active || i_row >= Sq) continue;
    const float inv = dvh / l;  // l carries the 256 of the P cast
    uint16_t* orow = out + ((int64_t)(b * Hq + h) * Sq + i_row) * D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const f32x4 y = o[dt][it] * inv;
      u32x2 w;
      if (out_f16) {
        w.x = __builtin_bit_cast(uint32_t, f16x2{(_Float16)y[0], (_Float16)y[1]});
        w.y = __builtin_bit_cast(uint32_t, f16x2{(_Float16)y[2], (_Float16)y[3]});
      } else {
        w.x = pack_bf16x2(y[0], y[1]);
        w.y = pack_bf16x2(y[2], y[3]);
      }
      *reinterpret_cast<u32x2*>(orow + 16 * dt) = w;
    }
  }
}

// the shapes the three entries serve; the reason of a refusal goes to the error message
int attn_check_shape(const char* fn, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D) {
  AO_REQUIRE(D == 64 || D == 128, "%s: head dimension D=%lld is not served (D must be 64 or 128)", fn, (long long)D);
  AO_REQUIRE(B >= 0 && Hq >= 0 && Hkv >= 0 && Sq >= 0 && Skv >= 0, "%s: negative size", fn);
  AO_REQUIRE(Hkv > 0 ? Hq % Hkv == 0 : Hq == 0, "%s: Hq=%lld must be a multiple of Hkv=%lld", fn, (long long)Hq, (long long)Hkv);
  AO_REQUIRE(B <= 65535 && Hq <= 65535, "%s: B=%lld and Hq=%lld must not exceed 65535", fn, (long long)B, (long long)Hq);
  AO_REQUIRE(Sq < (1ll << 23) && Skv < (1ll << 23), "%s: Sq=%lld and Skv=%lld must be below 2^23", fn, (long long)Sq, (long long)Skv);
  AO_REQUIRE(B * (Hq + 2 * Hkv) < (1ll << 31), "%s: B (Hq + 2 Hkv) must be below 2^31", fn);
  return AO_OK;
}

template <bool F16>
int attn_quantize_launch(const AttnCastArgs& a, float* state, float* descale, int64_t heads, int64_t chunks, hipStream_t stream) {
  ao::launch(fp8_attn_amax_kernel<F16>, dim3((unsigned)heads, (unsigned)chunks), dim3(kCastThreads), 0, stream, a, reinterpret_cast<uint32_t*>(state));
  AO_LAUNCH_CHECK("fp8_attn_amax_kernel launch");
  ao::launch(fp8_attn_cast_kernel<F16>, dim3((unsigned)heads, (unsigned)chunks), dim3(kCastThreads), 0, stream, a, (const float*)state, descale);
  AO_LAUNCH_CHECK("fp8_attn_cast_kernel launch");
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_fp8_attn_fits(int q_rank, const int64_t* q_shape, int k_rank, const int64_t* k_shape, int v_rank, const int64_t* v_shape) {
  const char* fn = __func__;
  auto refuse = [&](auto... args) { set_error(args...); return 0; };
  if (q_rank != 4 || k_rank != 4 || v_rank != 4)
    return refuse("%s: expected 4-D tensors [B, H, S, D], got ranks %d, %d, %d", fn, q_rank, k_rank, v_rank);
  if (!q_shape || !k_shape || !v_shape) return refuse("%s: null pointer argument", fn);
  for (int i = 0; i < 4; ++i)
    if (k_shape[i] != v_shape[i])
      return refuse("%s: K and V must have the same shape, got [%lld, %lld, %lld, %lld] and [%lld, %lld, %lld, %lld]", fn, (long long)k_shape[0],
                    (long long)k_shape[1], (long long)k_shape[2], (long long)k_shape[3], (long long)v_shape[0], (long long)v_shape[1],
                    (long long)v_shape[2], (long long)v_shape[3]);
  if (q_shape[0] != k_shape[0]) return refuse("%s: batch size mismatch: %lld and %lld", fn, (long long)q_shape[0], (long long)k_shape[0]);
  if (q_shape[3] != k_shape[3]) return refuse("%s: head dimension mismatch: %lld and %lld", fn, (long long)q_shape[3], (long long)k_shape[3]);
  return attn_check_shape(fn, q_shape[0], q_shape[1], k_shape[1], q_shape[2], k_shape[2], q_shape[3]) == AO_OK ? 1 : 0;
}

extern "C" int ao_fp8_attn_quantize(const void* q, const void* k, const void* v, const int64_t* q_strides, const int64_t* k_strides,
                                    const int64_t* v_strides, int is_fp16, float* state, uint8_t* q8, uint8_t* k8, uint8_t* v8, float* descale,
                                    int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, void* stream) {
  if (int rc = attn_check_shape(__func__, B, Hq, Hkv, Sq, Skv, D)) return rc;
  if (B == 0 || Hkv == 0 || (Sq == 0 && Skv == 0)) return AO_OK;
  AO_REQUIRE_PTR(q_strides);
  AO_REQUIRE_PTR(k_strides);
  AO_REQUIRE_PTR(v_strides);
  AO_REQUIRE_PTR(state);
  AO_REQUIRE_PTR(descale);
  AttnCastArgs a;
  const void* x[3] = {q, k, v};
  uint8_t* codes[3] = {q8, k8, v8};
  const int64_t* strides[3] = {q_strides, k_strides, v_strides};
  for (int t = 0; t < 3; ++t) {
    const int64_t S = t == 0 ? Sq : Skv;
    if (S > 0) {
      AO_REQUIRE_PTR(x[t]);
      AO_REQUIRE_PTR(codes[t]);
    }
    AO_REQUIRE(aligned_to(x[t], 16) && aligned_to(codes[t], 8) && strides[t][0] % 8 == 0 && strides[t][1] % 8 == 0 && strides[t][2] % 8 == 0 &&
                   strides[t][0] >= 0 && strides[t][1] >= 0 && strides[t][2] >= 0,
               "%s: tensor %d must be 16-byte aligned with non-negative batch / head / row strides that are multiples of 8 elements "
               "(the head dimension itself contiguous)", __func__, t);
    a.t[t] = AttnCastTensor{static_cast<const uint16_t*>(x[t]), codes[t], strides[t][0], strides[t][1], strides[t][2], (int)S,
                            (int)(t == 0 ? Hq : Hkv)};
  }
  a.B = (int)B, a.Hkv = (int)Hkv, a.groups = (int)(Hq / Hkv), a.D = (int)D;
  const int64_t heads = B * (Hq + 2 * Hkv), chunks = (std::max(Sq, Skv) + kCastRows - 1) / kCastRows;
  return is_fp16 ? attn_quantize_launch<true>(a, state, descale, heads, chunks, (hipStream_t)stream)
                 : attn_quantize_launch<false>(a, state, descale, heads, chunks, (hipStream_t)stream);
}

extern "C" int ao_fp8_attn_fwd(const uint8_t* q8, const uint8_t* k8, const uint8_t* v8, const float* dq, const float* dk, const float* dv, void* out,
                               int out_fp16, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, int is_causal, float scale,
                               void* stream) {
  if (int rc = attn_check_shape(__func__, B, Hq, Hkv, Sq, Skv, D)) return rc;
  if (B == 0 || Hq == 0 || Sq == 0) return AO_OK;
  AO_REQUIRE(Skv >= 1, "%s: Skv=0: there is no key to attend to", __func__);
  AO_REQUIRE(scale == scale && fabsf(scale) < INFINITY, "%s: scale must be finite", __func__);
  AO_REQUIRE_PTR(q8);
  AO_REQUIRE_PTR(k8);
  AO_REQUIRE_PTR(v8);
  AO_REQUIRE_PTR(dq);
  AO_REQUIRE_PTR(dk);
  AO_REQUIRE_PTR(dv);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(q8, 16) && aligned_to(k8, 16) && aligned_to(v8, 16) && aligned_to(out, 8),
             "%s: q8, k8 and v8 must be 16-byte aligned and out 8-byte aligned", __func__);
  const int nqt = (int)((Sq + kQTile - 1) / kQTile);
  const dim3 grid((unsigned)nqt, (unsigned)Hq, (unsigned)B);
  const float scale_log2e = scale * 1.4426950408889634f;
  auto go = [&](auto kernel) {
    ao::launch(kernel, grid, dim3(kAttnThreads), 0, (hipStream_t)stream, q8, k8, v8, dq, dk, dv, static_cast<uint16_t*>(out), out_fp16, (int)Hq,
               (int)Hkv, (int)Sq, (int)Skv, nqt, scale_log2e);
  };
  if (D == 128) { if (is_causal) go(fp8_attn_fwd_kernel<128, true>); else go(fp8_attn_fwd_kernel<128, false>); }
  else { if (is_causal) go(fp8_attn_fwd_kernel<64, true>); else go(fp8_attn_fwd_kernel<64, false>); }
  AO_LAUNCH_CHECK("fp8_attn_fwd_kernel launch");
  return AO_OK;
}
