// Intx weights (int1 .. int8, torchao/quantization/quantize_/workflows/intx) on gfx950: the fused affine cast, the bit-packed device layout, the
// per-token int8 fake quantization of the activation, and a bf16 x b-bit linear that decodes the weight in registers.
//
// The arithmetic is the reference's bf16 TENSOR arithmetic (quant_primitives.py:1534-1568 choose_qparams_affine, :480-482 quantize_affine,
// :854-857 dequantize_affine on a bf16 weight): every step one fp32 operation rounded once to bf16, divisions IEEE.
//   range    mn = min(min_group, 0), mx = max(max_group, 0)
//   scale    SYMMETRIC                   s = bf16(max(-mn, mx) / ((qmax - qmin) / 2))
//            SYMMETRIC_NO_CLIPPING_ERR   smin = bf16(mn / qmin), smax = bf16(mx / qmax), s = smin > smax ? smin : smax   (int1: qmax = 0, so
//                                        smax is Inf or NaN and is kept as it comes)
//            ASYMMETRIC                  s = bf16(bf16(mx - mn) / (qmax - qmin))
//            s = max(s, 2^-126) unless it is NaN (torch.clamp keeps NaN);  a NaN is stored as 0x7FC0
//   zero     symmetric: 0;  ASYMMETRIC: zp = clamp(bf16(qmin - rint(bf16(mn / s))), qmin, qmax)
//   code     q = clamp(bf16(rint(bf16(w * bf16(1 / s))) + zp), qmin, qmax), rint to even;  a NaN stores 0
//   decode   w = bf16((q - zp) * s): the integer is at most 255 in magnitude and s has 8 significant bits, so the fp32 product is exact
//   act      ASYMMETRIC int8 per row (token), then decode: the fake-quantized activation as bf16
//
// The packed layout.  u = q - qmin in [0, 2^b).  A row is cut into RUNS of 32 weights (K % 32 == 0; a group size is a
// multiple of 32, so a run has ONE scale and zero-point).  u is split into fields, low bits first: 3 = 2 + 1, 5 = 4 + 1, 6 = 4 + 2, 7 = 4 + 2 + 1.
// A run is b dwords: the 4-bit plane (4 dwords), then the 2-bit plane (2), then the 1-bit plane (1), as far as b has them.  Inside a plane of
// width f, dword d holds the 32 / f weights from 32 / f * d on, and weight 32 / f * d + 4 t + j sits in byte j at bit f * t: so
// `(dword >> f t) & mask` IS the four weights 4 t .. 4 t + 3 of that dword as four bytes, in k order, and the planes of one weight meet with
// one shift and one v_and_or_b32 each.  Four such bytes become four floats through v_cvt_f32_ubyte0..3.  b = 8 is the plain signed byte
// array (u = q ^ 0x80): one loader serves the unpacked tensor's qdata in place.
//
// The linear, y = x dequant(W)^T (+ bias), bf16 in and out, fp32 accumulation on v_mfma_f32_16x16x32_bf16, one rounding at the store.
// Lane (n = lane & 15, kq = lane >> 4) owns ONE run of a row per 128-k step: it loads b dwords, decodes 32 weights to four MFMA operands
// of 8 bf16, and multiplies them with x[m][32 run + 8 i ..] for i = 0 .. 3 (the k order inside an MFMA is free as long as both operands agree).
//   stream form  a workgroup owns 16 columns, its waves split the 128-k steps and request four steps ahead; scale and zero-point ride
//                with the weight request; the partial tiles meet in LDS in wave order (the frame of wo8_stream_kernel)
//   tiled form   64 x 64 output tiles, four waves of 32 x 32, K steps of 128: x as bf16 and W PACKED in LDS (b dwords a run) with the
//                run's (qmin - zp, s) staged once per K tile as two floats; decoded on the way to the MFMA
#include "common.h"
#include "quant_math.h"
#include "two_form_route.h"

#include <algorithm>

namespace ao {
namespace {

constexpr int kMapSym = AO_INTX_MAP_SYMMETRIC, kMapNoClip = AO_INTX_MAP_SYMMETRIC_NO_CLIPPING_ERR, kMapAsym = AO_INTX_MAP_ASYMMETRIC;
constexpr float kBf16Tiny = 1.17549435e-38f;  // 2^-126, torch.finfo(bfloat16).smallest_normal
constexpr uint16_t kBf16NaN = 0x7FC0;

__device__ __forceinline__ uint16_t intx_bf16_bits(float v) { return v != v ? kBf16NaN : f32_to_bf16_bits(v); }

// (mn, mx: the group's range with zero included) -> s, zp as bf16-valued floats
__device__ __forceinline__ void intx_qparams(int map, float mn, float mx, float qmin, float qmax, float& s, float& zp) {
  if (map == kMapAsym) {
    s = round_bf16(round_bf16(mx - mn) / (qmax - qmin));
    s = s != s ? s : fmaxf(s, kBf16Tiny);
    zp = round_bf16(qmin - rintf(round_bf16(mn / s)));
    zp = zp != zp ? 0.f : fminf(fmaxf(zp, qmin), qmax);
  } else {
    if (map == kMapSym) {
      s = round_bf16(fmaxf(-mn, mx) / ((qmax - qmin) * 0.5f));
    } else {
      const float smin = round_bf16(mn / qmin), smax = round_bf16(mx / qmax);
      s = smin > smax ? smin : smax;
    }
    s = s != s ? s : fmaxf(s, kBf16Tiny);
    zp = 0.f;
  }
}

__device__ __forceinline__ uint32_t intx_code(float w, float inv, float zp, float qmin, float qmax) {
  const float q = round_bf16(rintf(round_bf16(w * inv)) + zp);
  return q != q ? 0u : (uint32_t)(int)fminf(fmaxf(q, qmin), qmax) & 0xffu;
}

// ---- ao_intx_quantize ---------------------------------------------------------------------------------------------------------------
// The tensor is a flat run of groups (K % g == 0).  A group belongs to `lpg` adjacent lanes of a wave (a power of two dividing g / 8, at
// most 64), each of which walks g / 8 / lpg 16-byte pieces; a wave owns 64 / lpg groups in a row of the flat order.  Both reductions are
// butterflies inside the lanes of a group.  The second pass reads the pieces again (from cache).
struct IntxQuantArgs {
  const uint16_t* w;      // bf16 [N][K]
  int8_t* q;              // [N][K]
  uint16_t* scale;        // bf16 [N][K / g]
  int8_t* zp;             // [N][K / g]
  int64_t groups;         // N * K / g
  int g, lpg, map, given; // given: scale and zp are inputs (the custom scale / zero-point branch of from_hp)
  float qmin, qmax;
};

__global__ __launch_bounds__(kRowThreads) void intx_quantize_kernel(IntxQuantArgs p) {
  const int lane = threadIdx.x & 63, sl = lane & (p.lpg - 1);
  const int64_t wave = (int64_t)blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
  const int64_t gi = wave * (64 / p.lpg) + lane / p.lpg;
  const bool live = gi < p.groups;
  const int64_t gq = live ? gi : 0;  // (idle lanes walk group 0 and store nothing: the butterflies need every lane)
  const u32x4* src = reinterpret_cast<const u32x4*>(p.w + gq * p.g);
  const int pieces = p.g >> 3;
  float s, zp;
  if (p.given) {
    s = bf16_lo_to_f32(p.scale[gq]);
    zp = (float)p.zp[gq];
  } else {
    float mn = 0.f, mx = 0.f;
    for (int i = sl; i < pieces; i += p.lpg) {
      float f[8];
      unpack_bf16x8(src[i], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) mn = fminf(mn, f[j]), mx = fmaxf(mx, f[j]);
    }
    for (int off = 1; off < p.lpg; off <<= 1) {
      mn = fminf(mn, __shfl_xor(mn, off));
      mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    intx_qparams(p.map, mn, mx, p.qmin, p.qmax, s, zp);
    if (live && sl == 0) {
      p.scale[gi] = intx_bf16_bits(s);
      p.zp[gi] = (int8_t)(int)zp;
    }
  }
  if (!live) return;
  const float inv = round_bf16(1.0f / s);
  u32x2* dst = reinterpret_cast<u32x2*>(p.q + gi * p.g);
  for (int i = sl; i < pieces; i += p.lpg) {
    float f[8];
    unpack_bf16x8(src[i], f);
    uint32_t c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = intx_code(f[j], inv, zp, p.qmin, p.qmax);
    dst[i] = u32x2{c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24), c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24)};
  }
}

// ---- ao_int8_fake_quantize_per_token_asym: one workgroup a row, the second pass reads the row from cache --------------------------------
__global__ __launch_bounds__(kRowThreads) void intx_act_fake_quant_kernel(const uint16_t* x, uint16_t* out, int K) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const u32x4* xr = reinterpret_cast<const u32x4*>(x + row * K);
  u32x4* orow = reinterpret_cast<u32x4*>(out + row * K);
  const int nvec = K >> 3;
  float mn = 0.f, mx = 0.f;
  for (int i = threadIdx.x; i < nvec; i += kRowThreads) {
    float f[8];
    unpack_bf16x8(xr[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) mn = fminf(mn, f[j]), mx = fmaxf(mx, f[j]);
  }
  mx = block_max(mx, red);
  mn = -block_max(-mn, red);
  float s, zp;
  intx_qparams(kMapAsym, mn, mx, -128.f, 127.f, s, zp);
  const float inv = round_bf16(1.0f / s);
  for (int i = threadIdx.x; i < nvec; i += kRowThreads) {
    float f[8];
    unpack_bf16x8(xr[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float q = round_bf16(rintf(round_bf16(f[j] * inv)) + zp);
      f[j] = (fminf(fmaxf(q, -128.f), 127.f) - zp) * s;  // (q - zp exact; a NaN q reaches the output as NaN through s)
    }
    orow[i] = pack_bf16x8(f);
  }
}

// ---- pack / unpack: a thread a run -------------------------------------------------------------------------------------------------------
// the bytes of field (width F, at bit SH of u) of the four weights 4 t .. 4 t + 3 of plane dword `p`, moved to bit `SH` of each byte
template <int F, int SH>
__device__ __forceinline__ uint32_t intx_field4(uint32_t p, int t) {
  constexpr uint32_t mask = (((1u << F) - 1u) * 0x01010101u) << SH;
  const int right = F * t - SH;  // compile time after unrolling
  if (right >= 0) return (p >> right) & mask;
  return (p << (SH - F * t)) & mask;
}

// 32 codes u (bytes of u[8], k order) -> the run's B dwords
template <int B>
__device__ __forceinline__ void intx_pack_run(const uint32_t (&u)[8], uint32_t (&out)[B]) {
  int o = 0, sh = 0;
  auto plane = [&](auto width) {
    constexpr int F = decltype(width)::value;
#pragma unroll
    for (int d = 0; d < F; ++d) {
      uint32_t acc = 0;
#pragma unroll
      for (int t = 0; t < 8 / F; ++t) acc |= ((u[(8 / F) * d + t] >> sh) & (((1u << F) - 1u) * 0x01010101u)) << (F * t);
      out[o++] = acc;
    }
    sh += F;
  };
  if (B & 4) plane(std::integral_constant<int, 4>{});
  if (B & 2) plane(std::integral_constant<int, 2>{});
  if (B & 1) plane(std::integral_constant<int, 1>{});
}

// the run's B dwords -> 32 codes u as the bytes of u[8], k order (u[i]: weights 4 i .. 4 i + 3)
template <int B>
__device__ __forceinline__ void intx_unpack_run(const uint32_t (&in)[B], uint32_t (&u)[8]) {
  if (B == 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) u[i] = in[i] ^ 0x80808080u;
    return;
  }
  constexpr int o2 = (B & 4) ? 4 : 0, o1 = o2 + ((B & 2) ? 2 : 0);  // where the 2-bit and the 1-bit plane start
  constexpr int s2 = (B & 4) ? 4 : 0, s1 = s2 + ((B & 2) ? 2 : 0);  // where their fields sit in u
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint32_t v = 0;
    if (B & 4) v = intx_field4<4, 0>(in[i >> 1], i & 1);
    if (B & 2) v |= intx_field4<2, s2>(in[o2 + (i >> 2)], i & 3);
    if (B & 1) v |= intx_field4<1, s1>(in[o1], i);
    u[i] = v;
  }
}

template <int B>
__global__ __launch_bounds__(kRowThreads) void intx_pack_kernel(const int8_t* q, uint32_t* packed, int64_t runs) {
  const int64_t r = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  if (r >= runs) return;
  const u32x4* src = reinterpret_cast<const u32x4*>(q + r * 32);
  const u32x4 a = src[0], c = src[1];
  const uint32_t bias = 0x01010101u * (uint32_t)(1 << (B - 1));  // u = q - qmin: q + 2^(b-1) in every byte, no carry out of b bits
  uint32_t u[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w}, out[B];
  constexpr uint32_t keep = ((1u << B) - 1u) * 0x01010101u;
#pragma unroll
  for (int i = 0; i < 8; ++i) u[i] = (((u[i] & keep) ^ bias)) & keep;  // (q in range: adding 2^(b-1) mod 2^b flips bit b - 1)
  intx_pack_run<B>(u, out);
#pragma unroll
  for (int i = 0; i < B; ++i) packed[r * B + i] = out[i];
}

template <int B>
__global__ __launch_bounds__(kRowThreads) void intx_unpack_kernel(const uint32_t* packed, int8_t* q, int64_t runs) {
  const int64_t r = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  if (r >= runs) return;
  uint32_t in[B], u[8];
#pragma unroll
  for (int i = 0; i < B; ++i) in[i] = packed[r * B + i];
  intx_unpack_run<B>(in, u);
  // q = u + qmin: flip bit b - 1 and extend it through the byte
  constexpr uint32_t top = 0x01010101u * (1u << (B - 1)), ext = 0x01010101u * ((0xFFu << B) & 0xFFu);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t f = u[i] ^ top;                          // two's complement in b bits
    u[i] = f | (((f & top) >> (B - 1)) * 0xFFu & ext);      // bytes whose bit b - 1 is set get the bits above it
  }
  u32x4* dst = reinterpret_cast<u32x4*>(q + r * 32);
  dst[0] = u32x4{u[0], u[1], u[2], u[3]};
  dst[1] = u32x4{u[4], u[5], u[6], u[7]};
}

// ---- the decode: a run's dwords -> four MFMA operands of 8 bf16 (operand i: weights 8 i .. 8 i + 7) ------------------------------------------
// c = qmin - zp (an integer as a float), s the scale: w = bf16((u + c) * s), both fp32 operations exact
template <int B>
__device__ __forceinline__ void intx_decode_run(const uint32_t (&in)[B], float c, float s, u32x4 (&w)[4]) {
  uint32_t u[8];
  intx_unpack_run<B>(in, u);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t o[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t v = u[2 * i + h];
      const float f0 = (float)(v & 0xffu), f1 = (float)((v >> 8) & 0xffu), f2 = (float)((v >> 16) & 0xffu), f3 = (float)(v >> 24);
      o[2 * h] = pack_bf16x2((f0 + c) * s, (f1 + c) * s);
      o[2 * h + 1] = pack_bf16x2((f2 + c) * s, (f3 + c) * s);
    }
    w[i] = u32x4{o[0], o[1], o[2], o[3]};
  }
}

// ---- dequantize (from either layout): a thread a run ---------------------------------------------------------------------------------------
template <int B>
__global__ __launch_bounds__(kRowThreads) void intx_dequantize_kernel(const uint32_t* packed, const uint16_t* scale, const int8_t* zp, uint16_t* out,
                                                                       int64_t runs, int runs_per_group, float qmin) {
  const int64_t r = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  if (r >= runs) return;
  uint32_t in[B];
#pragma unroll
  for (int i = 0; i < B; ++i) in[i] = packed[r * B + i];
  const int64_t gi = r / runs_per_group;
  u32x4 w[4];
  intx_decode_run<B>(in, qmin - (float)zp[gi], bf16_lo_to_f32(scale[gi]), w);
  u32x4* dst = reinterpret_cast<u32x4*>(out + r * 32);
#pragma unroll
  for (int i = 0; i < 4; ++i) dst[i] = w[i];
}

// ---- the linear ----------------------------------------------------------------------------------------------------------------------------
// The seam starts at the weight-only 8-bit linear's (wo8_kernels.hip: 64 rows, the last count the stream form serves with one grid row).
constexpr int kStreamMaxRows = AO_INTX_LINEAR_STREAM_MAX_M;

thread_local int g_form = 0;  // ao_intx_linear_set_form: 0 the product route, 1 stream, 2 tile

const char* intx_shape_reason(int bits, int64_t M, int64_t N, int64_t K, int64_t g) {
  if (bits < 1 || bits > 8) return "bits must be 1 .. 8";
  if (M < 0 || N < 1 || K < 32) return "M >= 0, N >= 1 and K >= 32 are required";
  if (K % 32 != 0) return "K must be a multiple of 32 (a packed run is 32 weights)";
  if (g < 32 || g % 32 != 0 || K % g != 0) return "the group size must be a multiple of 32 that divides K";
  if (M >= (1ll << 31) || N >= (1ll << 31) || K > (1ll << 31) - 1024) return "M, N < 2^31 and K <= 2^31 - 1024 are required";
  if (M * K >= (1ll << 31) || N * K >= (1ll << 31) || M * N >= (1ll << 40)) return "x and W must hold fewer than 2^31 elements";
  return nullptr;
}

TwoFormRoute intx_route(int bits, int64_t M, int64_t N, int64_t K, int64_t g) {
  if (intx_shape_reason(bits, M, N, K, g) != nullptr) return TwoFormRoute{};
  TwoFormRoute r = two_form_route(g_form != 0 ? g_form : (M <= kStreamMaxRows ? 1 : 2), M, N, K, 64);
  r.grid_y = std::max(r.grid_y, 1);
  return r;
}

struct IntxLinearArgs {
  const uint16_t* x;      // bf16 [M][K]
  const uint32_t* w;      // [N][K / 32][B] dwords
  const uint16_t* scale;  // bf16 [N][K / g]
  const int8_t* zp;       // [N][K / g]
  const uint16_t* bias;   // bf16 [N] or null
  uint16_t* out;          // bf16 [M][N]
  int M, N, K;
  int rpg;                // runs a group: g / 32
  float qmin;
};

__device__ __forceinline__ f32x4 mfma_bf16(const u32x4& a, const u32x4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// a run's dwords, plane by plane: every load a whole dword or wider, 4-byte aligned
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
template <int B>
__device__ __forceinline__ void intx_load_run(const uint32_t* p, uint32_t (&d)[B]) {
  int o = 0;
  if (B == 8) {
    const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4_a4*>(p)), c = __builtin_nontemporal_load(reinterpret_cast<const u32x4_a4*>(p + 4));
    d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w, d[4 % B] = c.x, d[5 % B] = c.y, d[6 % B] = c.z, d[7 % B] = c.w;
    return;
  }
  if (B & 4) {
    const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4_a4*>(p));
    d[0] = a.x, d[1 % B] = a.y, d[2 % B] = a.z, d[3 % B] = a.w;
    o = 4;
  }
  if (B & 2) {
    const u32x2 a = __builtin_nontemporal_load(reinterpret_cast<const u32x2_a4*>(p + o));
    d[o % B] = a.x, d[(o + 1) % B] = a.y;
    o += 2;
  }
  if (B & 1) d[o % B] = __builtin_nontemporal_load(p + o);
}

constexpr int kChunk = 4;  // 128-k steps a wave requests at once

template <int B, int MT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void intx_stream_kernel(IntxLinearArgs p) {
  __shared__ f32x4 red[WAVES][MT][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kq = lane >> 4;
  const int n = blockIdx.x * 16 + (lane & 15);
  const int m0 = blockIdx.y * 16 * MT;
  const int runs = p.K >> 5, groups = runs / p.rpg;
  const int ksteps = (runs + 3) >> 2;
  const int ks0 = (ksteps * wave) / WAVES, ks1 = (ksteps * (wave + 1)) / WAVES;
  // columns past N read the last row (never stored); runs past K read the row's first run and are zeroed
  const int nr = min(n, p.N - 1);
  const uint32_t* wrow = p.w + (size_t)nr * runs * B;
  const uint16_t* srow = p.scale + (size_t)nr * groups;
  const int8_t* zrow = p.zp + (size_t)nr * groups;
  const uint16_t* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = m0 + mt * 16 + (lane & 15);
    xrow[mt] = p.x + (size_t)(row < p.M ? row : m0) * p.K;  // rows past M alias the tile's first row: outputs never stored
  }
  struct Stage {
    uint32_t d[B];
    uint16_t s;
    int8_t z;
  };
  auto issue = [&](Stage (&st)[kChunk], int step) {
#pragma unroll
    for (int d = 0; d < kChunk; ++d) {
      const int run = (step + d) * 4 + kq;
      const int r = run < runs ? run : 0;
      intx_load_run<B>(wrow + (size_t)r * B, st[d].d);
      st[d].s = srow[r / p.rpg];
      st[d].z = zrow[r / p.rpg];
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
        const int run = (step + d) * 4 + kq;
        const bool live = run < runs;
        const u32x4 z = {0u, 0u, 0u, 0u};
        u32x4 w[4] = {z, z, z, z};
        if (live) intx_decode_run<B>(cur[d].d, p.qmin - (float)cur[d].z, bf16_lo_to_f32(cur[d].s), w);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const u32x4* xp = reinterpret_cast<const u32x4*>(xrow[mt] + (live ? run * 32 : 0));
          u32x4 a[4] = {xp[0], xp[1], xp[2], xp[3]};
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[mt] = mfma_bf16(live ? a[i] : z, w[i], acc[mt]);
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
  const float bias = (p.bias != nullptr && n < p.N) ? bf16_lo_to_f32(p.bias[n]) : 0.f;
  for (int mt = wave; mt < MT; mt += WAVES) {
    f32x4 c = red[0][mt][lane];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) c += red[w][mt][lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + mt * 16 + 4 * kq + r;
      if (row < p.M && n < p.N) p.out[(size_t)row * p.N + n] = f32_to_bf16_bits(c[r] + bias);
    }
  }
}

// Tiled form.  LDS stage: x [64 rows][128 k] bf16, rows kTileRow bytes apart (256 + 16: the 16 rows of a ds_read_b128 spread over the banks);
// W [64 rows][4 runs][B dwords] packed; the runs' (qmin - zp, s) as float pairs [64][4].  Thread t stages four 16-byte pieces of x (row
// t >> 2, the 64 bytes at 64 (t & 3)) and ONE run of W (row t >> 2, run t & 3) with its pair.
constexpr int kTileRow = 272;
constexpr int kTileX = 64 * kTileRow;

template <int B>
__global__ __launch_bounds__(256) void intx_tile_kernel(IntxLinearArgs p) {
  __shared__ __attribute__((aligned(16))) char xs[kTileX];
  __shared__ uint32_t ws[64 * 4 * B];
  __shared__ f32x2 qs[64 * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int sr = tid >> 2, sp = tid & 3;
  const int runs = p.K >> 5, groups = runs / p.rpg;
  const bool arow_ok = m0 + sr < p.M, brow_ok = n0 + sr < p.N;
  const uint16_t* xa = p.x + (size_t)(arow_ok ? m0 + sr : 0) * p.K;
  const int nr = brow_ok ? n0 + sr : 0;
  const uint32_t* wb = p.w + (size_t)nr * runs * B;
  const uint16_t* srow = p.scale + (size_t)nr * groups;
  const int8_t* zrow = p.zp + (size_t)nr * groups;
  const int ksteps = (runs + 3) >> 2;
  const u32x4 z = {0u, 0u, 0u, 0u};
  u32x4 ga[4];
  uint32_t gw[B];
  f32x2 gq;
  auto fetch = [&](int step) {
    const int run = step * 4 + sp;
    const bool kv = run < runs;  // (a run lies inside K or outside)
    const u32x4* xp = reinterpret_cast<const u32x4*>(xa + (kv ? run * 32 : 0));
#pragma unroll
    for (int i = 0; i < 4; ++i) ga[i] = (kv && arow_ok) ? xp[i] : z;
    const int r = kv ? run : 0;
    intx_load_run<B>(wb + (size_t)r * B, gw);
    // rows past N and runs past K decode to zero: code bytes kept, c = -u is not expressible, so s = 0 (finite codes times zero)
    gq = f32x2{p.qmin - (float)zrow[r / p.rpg], (kv && brow_ok) ? bf16_lo_to_f32(srow[r / p.rpg]) : 0.f};
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  fetch(0);
  for (int step = 0; step < ksteps; ++step) {
    __syncthreads();  // every wave is done with the previous stage
    u32x4* sa = reinterpret_cast<u32x4*>(xs + sr * kTileRow + sp * 64);
#pragma unroll
    for (int i = 0; i < 4; ++i) sa[i] = ga[i];
#pragma unroll
    for (int i = 0; i < B; ++i) ws[(sr * 4 + sp) * B + i] = gw[i];
    qs[sr * 4 + sp] = gq;
    __syncthreads();
    if (step + 1 < ksteps) fetch(step + 1);  // in flight under the MFMAs
    u32x4 bf[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int slot = (wn + 16 * j + (lane & 15)) * 4 + kq;
      uint32_t in[B];
#pragma unroll
      for (int i = 0; i < B; ++i) in[i] = ws[slot * B + i];
      const f32x2 q = qs[slot];
      intx_decode_run<B>(in, q.x, q.y, bf[j]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const u32x4* ap = reinterpret_cast<const u32x4*>(xs + (wm + 16 * i + (lane & 15)) * kTileRow + kq * 64);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const u32x4 af = ap[e];
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma_bf16(af, bf[j][e], acc[i][j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + 16 * j + (lane & 15);
    if (n >= p.N) continue;
    const float bias = p.bias != nullptr ? bf16_lo_to_f32(p.bias[n]) : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + 16 * i + 4 * kq + r;
        if (row < p.M) p.out[(size_t)row * p.N + n] = f32_to_bf16_bits(acc[i][j][r] + bias);
      }
  }
}

// ---- launches --------------------------------------------------------------------------------------------------------------------------------
template <typename F>
int with_bits(int bits, F&& f) {
  switch (bits) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

int check_bits(const char* fn, int bits) {
  AO_REQUIRE(bits >= 1 && bits <= 8, "%s: bits must be 1 .. 8, got %d", fn, bits);
  return AO_OK;
}

int check_runs(const char* fn, int64_t N, int64_t K) {
  if (int rc = check_rows(fn, N, K, 32)) return rc;
  AO_REQUIRE(N * K < (1ll << 40), "%s: N=%lld K=%lld too large", fn, (long long)N, (long long)K);
  return AO_OK;
}

unsigned blocks_for(int64_t items) { return (unsigned)((items + kRowThreads - 1) / kRowThreads); }

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_intx_quantize(const uint16_t* w, int8_t* q, uint16_t* scale, int8_t* zero_point, int64_t N, int64_t K, int64_t group_size,
                                int bits, int mapping, int qparams_given, void* stream) {
  if (int rc = check_bits(__func__, bits)) return rc;
  AO_REQUIRE(mapping >= kMapSym && mapping <= kMapAsym, "%s: mapping must be 0 (SYMMETRIC), 1 (SYMMETRIC_NO_CLIPPING_ERR) or 2 (ASYMMETRIC), got %d",
             __func__, mapping);
  if (int rc = check_rows(__func__, N, K, 8)) return rc;
  AO_REQUIRE(group_size >= 8 && group_size % 8 == 0 && K % group_size == 0 && group_size < (1ll << 31),
             "%s: group_size=%lld must be a multiple of 8 that divides K=%lld", __func__, (long long)group_size, (long long)K);
  AO_REQUIRE(N * K < (1ll << 40), "%s: N=%lld K=%lld too large", __func__, (long long)N, (long long)K);
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(scale);
  AO_REQUIRE_PTR(zero_point);
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(q, 8) && aligned_to(scale, 2), "%s: w must be 16-byte, q 8-byte and scale 2-byte aligned", __func__);
  int lpg = 1;
  while (lpg < 64 && (group_size / 8) % (lpg * 2) == 0) lpg *= 2;
  const int64_t groups = N * (K / group_size);
  const int64_t waves = (groups + 64 / lpg - 1) / (64 / lpg);
  const IntxQuantArgs a{w, q, scale, zero_point, groups, (int)group_size, lpg, mapping, qparams_given ? 1 : 0, (float)-(1 << (bits - 1)),
                        (float)((1 << (bits - 1)) - 1)};
  ao::launch(intx_quantize_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(kRowThreads), 0, (hipStream_t)stream, a);
  AO_LAUNCH_CHECK("intx_quantize_kernel launch");
  return AO_OK;
}

extern "C" int ao_int8_fake_quantize_per_token_asym(const uint16_t* x, uint16_t* out, int64_t M, int64_t K, void* stream) {
  if (int rc = check_rows(__func__, M, K, 8)) return rc;
  AO_REQUIRE(K <= (1ll << 24), "%s: K=%lld too large", __func__, (long long)K);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(out, 16), "%s: x and out must be 16-byte aligned", __func__);
  ao::launch(intx_act_fake_quant_kernel, dim3((unsigned)M), dim3(kRowThreads), 0, (hipStream_t)stream, x, out, (int)K);
  AO_LAUNCH_CHECK("intx_act_fake_quant_kernel launch");
  return AO_OK;
}

extern "C" int ao_intx_pack(const int8_t* q, uint32_t* packed, int64_t N, int64_t K, int bits, void* stream) {
  if (int rc = check_bits(__func__, bits)) return rc;
  if (int rc = check_runs(__func__, N, K)) return rc;
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(packed);
  AO_REQUIRE(aligned_to(q, 16) && aligned_to(packed, 4), "%s: q must be 16-byte and packed 4-byte aligned", __func__);
  const int64_t runs = N * (K / 32);
  if (bits == 8) {  // the plain byte array
    hipError_t e = hipMemcpyAsync(packed, q, (size_t)(N * K), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return hip_failed(e, "ao_intx_pack copy");
    return AO_OK;
  }
  with_bits(bits, [&](auto b) {
    ao::launch(intx_pack_kernel<decltype(b)::value>, dim3(blocks_for(runs)), dim3(kRowThreads), 0, (hipStream_t)stream, q, packed, runs);
    return 0;
  });
  AO_LAUNCH_CHECK("intx_pack_kernel launch");
  return AO_OK;
}

extern "C" int ao_intx_unpack(const uint32_t* packed, int8_t* q, int64_t N, int64_t K, int bits, void* stream) {
  if (int rc = check_bits(__func__, bits)) return rc;
  if (int rc = check_runs(__func__, N, K)) return rc;
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(packed);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE(aligned_to(packed, 4) && aligned_to(q, 16), "%s: packed must be 4-byte and q 16-byte aligned", __func__);
  const int64_t runs = N * (K / 32);
  if (bits == 8) {
    hipError_t e = hipMemcpyAsync(q, packed, (size_t)(N * K), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return hip_failed(e, "ao_intx_unpack copy");
    return AO_OK;
  }
  with_bits(bits, [&](auto b) {
    ao::launch(intx_unpack_kernel<decltype(b)::value>, dim3(blocks_for(runs)), dim3(kRowThreads), 0, (hipStream_t)stream, packed, q, runs);
    return 0;
  });
  AO_LAUNCH_CHECK("intx_unpack_kernel launch");
  return AO_OK;
}

extern "C" int ao_intx_dequantize(const uint32_t* packed, const uint16_t* scale, const int8_t* zero_point, uint16_t* out, int64_t N, int64_t K,
                                  int64_t group_size, int bits, void* stream) {
  if (int rc = check_bits(__func__, bits)) return rc;
  if (int rc = check_runs(__func__, N, K)) return rc;
  AO_REQUIRE(group_size >= 32 && group_size % 32 == 0 && K % group_size == 0, "%s: group_size=%lld must be a multiple of 32 that divides K=%lld",
             __func__, (long long)group_size, (long long)K);
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(packed);
  AO_REQUIRE_PTR(scale);
  AO_REQUIRE_PTR(zero_point);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(packed, 4) && aligned_to(out, 16) && aligned_to(scale, 2), "%s: packed must be 4-byte, out 16-byte and scale 2-byte aligned", __func__);
  const int64_t runs = N * (K / 32);
  // qmin of the LAYOUT, -2^(bits - 1): the b = 8 loader reads u = q + 128 whatever range the codes keep to
  const float qmin = (float)-(1 << (bits - 1));
  with_bits(bits, [&](auto b) {
    ao::launch(intx_dequantize_kernel<decltype(b)::value>, dim3(blocks_for(runs)), dim3(kRowThreads), 0, (hipStream_t)stream, packed, scale,
               zero_point, out, runs, (int)(group_size / 32), qmin);
    return 0;
  });
  AO_LAUNCH_CHECK("intx_dequantize_kernel launch");
  return AO_OK;
}

extern "C" int ao_intx_linear_fits(int bits, int64_t M, int64_t N, int64_t K, int64_t group_size) {
  const char* why = intx_shape_reason(bits, M, N, K, group_size);
  if (why != nullptr) set_error("%s: %s (bits=%d M=%lld N=%lld K=%lld group_size=%lld)", __func__, why, bits, (long long)M, (long long)N, (long long)K,
                                (long long)group_size);
  return why == nullptr ? 1 : 0;
}

extern "C" int ao_intx_linear_route(int bits, int64_t M, int64_t N, int64_t K, int64_t group_size, int32_t* out, int cap) {
  return route_export(__func__, intx_route(bits, M, N, K, group_size), out, cap);
}

extern "C" int ao_intx_linear_set_form(int form) { return set_forced_form(__func__, form, g_form); }

extern "C" int ao_intx_linear(const uint16_t* x, const uint32_t* w, const uint16_t* scale, const int8_t* zero_point, const uint16_t* bias, uint16_t* out,
                              int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, void* stream) {
  const char* why = intx_shape_reason(bits, M, N, K, group_size);
  AO_REQUIRE(why == nullptr, "%s: %s (bits=%d M=%lld N=%lld K=%lld group_size=%lld)", __func__, why, bits, (long long)M, (long long)N, (long long)K,
             (long long)group_size);
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(scale);
  AO_REQUIRE_PTR(zero_point);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(w, 4), "%s: x must be 16-byte and w 4-byte aligned", __func__);
  AO_REQUIRE(aligned_to(scale, 2) && aligned_to(bias, 2) && aligned_to(out, 2), "%s: scale, bias and out must be 2-byte aligned", __func__);
  const TwoFormRoute r = intx_route(bits, M, N, K, group_size);
  AO_REQUIRE(r.kernel != 0, "%s: no route for M=%lld N=%lld K=%lld", __func__, (long long)M, (long long)N, (long long)K);
  const IntxLinearArgs a{x, w, scale, zero_point, bias, out, (int)M, (int)N, (int)K, (int)(group_size / 32), (float)-(1 << (bits - 1))};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return with_bits(bits, [&](auto b) {
    constexpr int B = decltype(b)::value;
    if (r.kernel == 1)
      return launch_stream_form<false>("intx_stream_kernel", "intx_stream_kernel launch", r, a, st, [](auto mt, auto waves) {
        return intx_stream_kernel<B, decltype(mt)::value, decltype(waves)::value>;
      });
    return launch_tile_form(intx_tile_kernel<B>, "intx_tile_kernel launch", r, a, st);
  });
}
