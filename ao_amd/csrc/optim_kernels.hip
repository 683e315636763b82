// Low-bit optimizers for gfx950: block-quantized Adam moments (8-bit and 4-bit table codes, e4m3 codes, or plain moments in the parameter's
// dtype) and the Adam / AdamW step of one parameter in ONE launch.
//
// Replaces, of torchao/optim: single_param_adam (adam.py:163-209), which the reference runs through torch.compile (Triton on ROCm) and
// which in eager mode is a chain of some forty launches a parameter, and the subclasses' copy_ / dequantize.  The arithmetic contract is
// stated once, in quant_math.h ("low-bit optimizer states"): the bytes are those of the reference's eager CPU run.
//
// One layout for the three kernels: 256 lanes, 16 consecutive elements a lane (16 bytes of 8-bit codes, 8 of 4-bit, 2 x 16 of bf16, 4 x 16 of
// fp32), so a workgroup takes a TILE of 4096 elements per trip: a multiple of every block size, a quantization block is never split
// across workgroups.  A block of B elements is B / 16 adjacent lanes: 4 .. 64 lanes meet by a butterfly of lane shuffles (no LDS, no
// barrier: the defaults 256 and 128 are 16 and 8 lanes), B = 2048 is two waves that meet through four LDS words.  The grid is
// min(tiles, cap) workgroups that walk the tiles in a strided loop; the bytes of a tile depend on nothing but the tile.  The tables go
// to LDS once a workgroup (3 KiB for the 8-bit triple); a code costs 8 + 2 dependent LDS reads, the 16 elements of a lane independent
// of one another.  No atomics.  In place: a lane reads its own codes before it writes them; the lanes of a block read the old scale
// before the reduction that the one writing lane waits for.
#include "common.h"
#include "quant_math.h"

#include <algorithm>

namespace ao {
namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 16;
constexpr int64_t kTile = (int64_t)kThreads * kPerLane;  // 4096 elements
constexpr int kGridCap = 2048;                           // 8 workgroups (32 waves) a CU on 256 CUs

enum Kind { K_Q8 = 0, K_Q4 = 1, K_FP8 = 2, K_PLAIN = 3 };

struct Moment {
  void* codes;  // K_PLAIN: the moment itself, in the parameter's dtype
  float* scale;
  const float* qmap;
};

struct StepArgs {
  void* p;
  const void* g;
  Moment m, v, vmax;
  int64_t n, tiles;
  int lb;  // log2 block size (quantized kinds)
  ao_optim_scalars s;
  int is_adamw, has_vmax, sr;
  uint32_t k0, k1, step, param;
};

struct CastArgs {
  const void* src;  // quantize: the values; dequantize: unused
  void* dst;        // dequantize: the values
  Moment q;
  int64_t n, tiles;
  int lb;
};

// 16 consecutive elements at `base` of a bf16 / fp32 array -> fp32; cnt < 16: the array ends inside the lane's run (plain states only)
template <bool BF16>
__device__ __forceinline__ void load16(const void* ptr, int64_t base, int cnt, float (&o)[16]) {
  if (cnt == 16) {
    if (BF16) {
      const u32x4* q = reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(ptr) + base);
      const u32x4 a = q[0], b = q[1];
      const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        o[2 * i] = bf16_lo_to_f32(w[i]);
        o[2 * i + 1] = bf16_hi_to_f32(w[i]);
      }
    } else {
      const f32x4* q = reinterpret_cast<const f32x4*>(static_cast<const float*>(ptr) + base);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 t = q[i];
        o[4 * i] = t.x;
        o[4 * i + 1] = t.y;
        o[4 * i + 2] = t.z;
        o[4 * i + 3] = t.w;
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    o[i] = 0.f;
    if (i < cnt) o[i] = BF16 ? bf16_lo_to_f32(static_cast<const uint16_t*>(ptr)[base + i]) : static_cast<const float*>(ptr)[base + i];
  }
}

// fp32 -> the array's dtype, RNE
template <bool BF16>
__device__ __forceinline__ void store16(void* ptr, int64_t base, int cnt, const float (&v)[16]) {
  if (cnt == 16) {
    if (BF16) {
      uint32_t w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
      u32x4* q = reinterpret_cast<u32x4*>(static_cast<uint16_t*>(ptr) + base);
      q[0] = u32x4{w[0], w[1], w[2], w[3]};
      q[1] = u32x4{w[4], w[5], w[6], w[7]};
    } else {
      f32x4* q = reinterpret_cast<f32x4*>(static_cast<float*>(ptr) + base);
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = f32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < cnt) {
      if (BF16)
        static_cast<uint16_t*>(ptr)[base + i] = f32_to_bf16_bits(v[i]);
      else
        static_cast<float*>(ptr)[base + i] = v[i];
    }
}

// bf16 bits of 16 values (the SR store)
__device__ __forceinline__ void store16_bits(void* ptr, int64_t base, int cnt, const uint32_t (&b)[16]) {
  if (cnt == 16) {
    u32x4* q = reinterpret_cast<u32x4*>(static_cast<uint16_t*>(ptr) + base);
    q[0] = u32x4{b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16)};
    q[1] = u32x4{b[8] | (b[9] << 16), b[10] | (b[11] << 16), b[12] | (b[13] << 16), b[14] | (b[15] << 16)};
    return;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < cnt) static_cast<uint16_t*>(ptr)[base + i] = (uint16_t)b[i];
}

// the lane's 16 values of one moment, dequantized (active: the lane holds elements; a quantized lane holds 16 or none)
template <int KIND, bool BF16>
__device__ __forceinline__ void decode16(const Moment& q, int64_t base, int cnt, int lb, const float* tab, float (&o)[16]) {
#pragma clang fp contract(off)
  if (KIND == K_PLAIN) {
    load16<BF16>(q.codes, base, cnt, o);
    return;
  }
  if (cnt == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
    return;
  }
  const float s = q.scale[base >> lb];
  if (KIND == K_Q4) {
    const u32x2 c = *reinterpret_cast<const u32x2*>(static_cast<const uint8_t*>(q.codes) + (base >> 1));
    const uint32_t w[2] = {c.x, c.y};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
      o[2 * i] = tab[b >> 4] * s;
      o[2 * i + 1] = tab[b & 15u] * s;
    }
    return;
  }
  const u32x4 c = *reinterpret_cast<const u32x4*>(static_cast<const uint8_t*>(q.codes) + base);
  const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (KIND == K_Q8) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[4 * i + j] = tab[(w[i] >> (8 * j)) & 0xffu] * s;
    } else {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
      o[4 * i] = lo.x * s;
      o[4 * i + 1] = lo.y * s;
      o[4 * i + 2] = hi.x * s;
      o[4 * i + 3] = hi.y * s;
    }
  }
}

__device__ __forceinline__ float amax16(const float (&v)[16]) {
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) a = fmaxf(a, fabsf(v[i]));
  return a;
}

// the maximum over the 2^(lb - 4) adjacent lanes of a block, in every one of them.  Up to 64 lanes: shuffles.  128 lanes (B = 2048): the two
// waves of the block (wave, wave ^ 1) meet in LDS; lb is uniform, so every lane of the workgroup reaches the barriers.
__device__ __forceinline__ float block_max(float x, int lb, float* red) {
  const int lanes = 1 << (lb - 4);
  for (int off = 1; off < min(lanes, kWave); off <<= 1) x = fmaxf(x, __shfl_xor(x, off));
  if (lanes > kWave) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = x;
    __syncthreads();
    x = fmaxf(red[wave], red[wave ^ 1]);
    __syncthreads();
  }
  return x;
}

// the lane's 16 fp32 values of one moment -> codes and (from the block's first lane) the scale; amax: the block's
template <int KIND>
__device__ __forceinline__ void encode16(const Moment& q, int64_t base, int lb, const float* tab, const float (&x)[16], float amax) {
#pragma clang fp contract(off)
  const float s = KIND == K_FP8 ? optim_fp8_scale(amax) : optim_block_scale(amax);
  if ((base & ((1ll << lb) - 1)) == 0) q.scale[base >> lb] = s;
  if (KIND == K_Q4) {
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t hi = optim_table_code<4>(x[2 * i] / s, tab), lo = optim_table_code<4>(x[2 * i + 1] / s, tab);
      w[i >> 2] |= ((hi << 4) | lo) << (8 * (i & 3));
    }
    *reinterpret_cast<u32x2*>(static_cast<uint8_t*>(q.codes) + (base >> 1)) = u32x2{w[0], w[1]};
    return;
  }
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (KIND == K_Q8) {
      w[i] = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[i] |= optim_table_code<8>(x[4 * i + j] / s, tab) << (8 * j);
    } else {
      w[i] = cvt4_e4m3(x[4 * i] / s, x[4 * i + 1] / s, x[4 * i + 2] / s, x[4 * i + 3] / s);
    }
  }
  *reinterpret_cast<u32x4*>(static_cast<uint8_t*>(q.codes) + base) = u32x4{w[0], w[1], w[2], w[3]};
}

template <int KIND>
__device__ __forceinline__ void load_table(float* tab, const float* qmap) {
  constexpr int T = KIND == K_Q8 ? 256 : 16;
  if (KIND == K_Q8 || KIND == K_Q4)
    if ((int)threadIdx.x < T && qmap != nullptr) tab[threadIdx.x] = qmap[threadIdx.x];
}

// ---- the step ---------------------------------------------------------------------------------------------------------------------------
template <int KIND, bool BF16>
__global__ __launch_bounds__(kThreads) void optim_adam_kernel(const StepArgs a) {
  __shared__ float tab[3][256];
  __shared__ float red[3][4];
  load_table<KIND>(tab[0], a.m.qmap);
  load_table<KIND>(tab[1], a.v.qmap);
  load_table<KIND>(tab[2], a.has_vmax ? a.vmax.qmap : nullptr);
  __syncthreads();
  const bool has_vmax = a.has_vmax != 0, is_adamw = a.is_adamw != 0;
  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int64_t base = tile * kTile + (int64_t)threadIdx.x * kPerLane;
    const int cnt = (int)std::min<int64_t>(std::max<int64_t>(a.n - base, 0), kPerLane);
    float p[16], g[16], m[16], v[16], vm[16];
    load16<BF16>(a.p, base, cnt, p);
    load16<BF16>(a.g, base, cnt, g);
    decode16<KIND, BF16>(a.m, base, cnt, a.lb, tab[0], m);
    decode16<KIND, BF16>(a.v, base, cnt, a.lb, tab[1], v);
    if (has_vmax) {
      decode16<KIND, BF16>(a.vmax, base, cnt, a.lb, tab[2], vm);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) vm[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < cnt) optim_adam_element(p[i], g[i], m[i], v[i], vm[i], has_vmax, is_adamw, a.s);

    if (BF16 && a.sr) {
      uint32_t b[16];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint64_t grp = (uint64_t)(base >> 3) + h;
        const Philox4 rnd = philox4x32_10((uint32_t)grp, (uint32_t)(grp >> 32), a.step, a.param, a.k0, a.k1);
#pragma unroll
        for (int j = 0; j < 8; ++j) b[8 * h + j] = optim_sr_bf16(p[8 * h + j], (rnd.w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
      }
      store16_bits(a.p, base, cnt, b);
    } else {
      store16<BF16>(a.p, base, cnt, p);
    }

    if (KIND == K_PLAIN) {
      store16<BF16>(a.m.codes, base, cnt, m);
      store16<BF16>(a.v.codes, base, cnt, v);
      if (has_vmax) store16<BF16>(a.vmax.codes, base, cnt, vm);
    } else {
      // (a lane past n holds zeros: it joins the reductions of blocks that do not exist and writes nothing)
      const float am = block_max(amax16(m), a.lb, red[0]);
      const float av = block_max(amax16(v), a.lb, red[1]);
      const float avm = has_vmax ? block_max(amax16(vm), a.lb, red[2]) : 0.f;
      if (cnt != 0) {
        encode16<KIND>(a.m, base, a.lb, tab[0], m, am);
        encode16<KIND>(a.v, base, a.lb, tab[1], v, av);
        if (has_vmax) encode16<KIND>(a.vmax, base, a.lb, tab[2], vm, avm);
      }
    }
  }
}

// ---- the casts ----------------------------------------------------------------------------------------------------------------------------
template <int KIND, bool BF16>
__global__ __launch_bounds__(kThreads) void optim_quantize_kernel(const CastArgs a) {
  __shared__ float tab[256];
  __shared__ float red[4];
  load_table<KIND>(tab, a.q.qmap);
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int64_t base = tile * kTile + (int64_t)threadIdx.x * kPerLane;
    const int cnt = base < a.n ? kPerLane : 0;
    float x[16];
    load16<BF16>(a.src, base, cnt, x);
    const float am = block_max(amax16(x), a.lb, red);
    if (cnt != 0) encode16<KIND>(a.q, base, a.lb, tab, x, am);
  }
}

template <int KIND, bool BF16>
__global__ __launch_bounds__(kThreads) void optim_dequantize_kernel(const CastArgs a) {
  __shared__ float tab[256];
  load_table<KIND>(tab, a.q.qmap);
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int64_t base = tile * kTile + (int64_t)threadIdx.x * kPerLane;
    if (base >= a.n) continue;
    float x[16];
    decode16<KIND, false>(a.q, base, kPerLane, a.lb, tab, x);
    store16<BF16>(a.dst, base, kPerLane, x);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }
int64_t grid_of(int64_t tiles, int max_workgroups) { return std::min<int64_t>(tiles, max_workgroups > 0 ? max_workgroups : kGridCap); }

int log2_block(int block_size) {
  for (int lb = 6; lb <= 11; ++lb)
    if (block_size == (1 << lb)) return lb;
  return -1;
}

int kind_of(int format) {
  switch (format) {
    case AO_OPTIM_Q8_SIGNED:
    case AO_OPTIM_Q8_UNSIGNED:
      return K_Q8;
    case AO_OPTIM_Q4_SIGNED:
    case AO_OPTIM_Q4_UNSIGNED:
      return K_Q4;
    case AO_OPTIM_FP8:
      return K_FP8;
    case AO_OPTIM_PLAIN:
      return K_PLAIN;
  }
  return -1;
}

int check_quantized(const char* fn, int64_t n, int block_size, int kind) {
  AO_REQUIRE(kind == K_Q8 || kind == K_Q4 || kind == K_FP8, "%s: format must be one of the AO_OPTIM_Q8 / Q4 / FP8 formats", fn);
  AO_REQUIRE(log2_block(block_size) >= 0, "%s: block_size must be a power of two from 64 to 2048, got %d", fn, block_size);
  AO_REQUIRE(n >= 0 && n < (1ll << 40), "%s: n=%lld must be in [0, 2^40)", fn, (long long)n);
  AO_REQUIRE(n % block_size == 0, "%s: n=%lld must be a multiple of block_size=%d", fn, (long long)n, block_size);
  return AO_OK;
}

int check_moment(const char* fn, const char* what, const Moment& q, int kind) {
  AO_REQUIRE(q.codes != nullptr, "%s: null pointer argument '%s_codes'", fn, what);
  AO_REQUIRE(aligned_to(q.codes, 16), "%s: %s_codes must be 16-byte aligned", fn, what);
  if (kind == K_PLAIN) return AO_OK;
  AO_REQUIRE(q.scale != nullptr, "%s: null pointer argument '%s_scale'", fn, what);
  AO_REQUIRE(kind == K_FP8 || q.qmap != nullptr, "%s: null pointer argument '%s_qmap'", fn, what);
  return AO_OK;
}

template <template <int, bool> class L, typename A>
void dispatch(int kind, bool bf16, const A& a, dim3 grid, hipStream_t st) {
  switch (kind * 2 + (bf16 ? 1 : 0)) {
    case 0: L<K_Q8, false>::go(a, grid, st); break;
    case 1: L<K_Q8, true>::go(a, grid, st); break;
    case 2: L<K_Q4, false>::go(a, grid, st); break;
    case 3: L<K_Q4, true>::go(a, grid, st); break;
    case 4: L<K_FP8, false>::go(a, grid, st); break;
    case 5: L<K_FP8, true>::go(a, grid, st); break;
    case 6: L<K_PLAIN, false>::go(a, grid, st); break;
    default: L<K_PLAIN, true>::go(a, grid, st); break;
  }
}
template <int KIND, bool BF16>
struct StepLaunch {
  static void go(const StepArgs& a, dim3 grid, hipStream_t st) { launch(optim_adam_kernel<KIND, BF16>, grid, dim3(kThreads), 0, st, a); }
};
template <int KIND, bool BF16>
struct QuantLaunch {
  static void go(const CastArgs& a, dim3 grid, hipStream_t st) {
    if (KIND != K_PLAIN) launch(optim_quantize_kernel<KIND == K_PLAIN ? K_Q8 : KIND, BF16>, grid, dim3(kThreads), 0, st, a);
  }
};
template <int KIND, bool BF16>
struct DequantLaunch {
  static void go(const CastArgs& a, dim3 grid, hipStream_t st) {
    if (KIND != K_PLAIN) launch(optim_dequantize_kernel<KIND == K_PLAIN ? K_Q8 : KIND, BF16>, grid, dim3(kThreads), 0, st, a);
  }
};

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_optim_grid(int64_t n, int max_workgroups, int64_t* out) {
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(n >= 0 && n < (1ll << 40), "%s: n=%lld must be in [0, 2^40)", __func__, (long long)n);
  AO_REQUIRE(max_workgroups >= 0, "%s: max_workgroups=%d must not be negative", __func__, max_workgroups);
  out[0] = kTile;
  out[1] = tiles_of(n);
  out[2] = grid_of(out[1], max_workgroups);
  return AO_OK;
}

extern "C" int ao_optim_quantize(const void* src, int src_bf16, void* codes, float* scale, const float* qmap, int64_t n, int block_size,
                                 int format, void* stream) {
  const int kind = kind_of(format);
  if (int rc = check_quantized(__func__, n, block_size, kind)) return rc;
  if (n == 0) return AO_OK;
  AO_REQUIRE_PTR(src);
  AO_REQUIRE(aligned_to(src, 16), "%s: src must be 16-byte aligned", __func__);
  CastArgs a{};
  a.src = src;
  a.q = Moment{codes, scale, qmap};
  if (int rc = check_moment(__func__, "the", a.q, kind)) return rc;
  a.n = n;
  a.tiles = tiles_of(n);
  a.lb = log2_block(block_size);
  dispatch<QuantLaunch>(kind, src_bf16 != 0, a, dim3((unsigned)grid_of(a.tiles, 0)), (hipStream_t)stream);
  AO_LAUNCH_CHECK("optim_quantize_kernel launch");
  return AO_OK;
}

extern "C" int ao_optim_dequantize(const void* codes, const float* scale, const float* qmap, void* dst, int dst_bf16, int64_t n,
                                   int block_size, int format, void* stream) {
  const int kind = kind_of(format);
  if (int rc = check_quantized(__func__, n, block_size, kind)) return rc;
  if (n == 0) return AO_OK;
  AO_REQUIRE_PTR(dst);
  AO_REQUIRE(aligned_to(dst, 16), "%s: dst must be 16-byte aligned", __func__);
  CastArgs a{};
  a.dst = dst;
  a.q = Moment{const_cast<void*>(codes), const_cast<float*>(scale), qmap};
  if (int rc = check_moment(__func__, "the", a.q, kind)) return rc;
  a.n = n;
  a.tiles = tiles_of(n);
  a.lb = log2_block(block_size);
  dispatch<DequantLaunch>(kind, dst_bf16 != 0, a, dim3((unsigned)grid_of(a.tiles, 0)), (hipStream_t)stream);
  AO_LAUNCH_CHECK("optim_dequantize_kernel launch");
  return AO_OK;
}

extern "C" int ao_optim_adam_step(void* p, const void* grad, int bf16, void* m_codes, float* m_scale, const float* m_qmap, void* v_codes,
                                  float* v_scale, const float* v_qmap, void* vmax_codes, float* vmax_scale, const float* vmax_qmap,
                                  int format, int64_t n, int block_size, const ao_optim_scalars* scalars, int is_adamw, int sr, int64_t seed,
                                  int64_t step, int64_t param_index, int max_workgroups, void* stream) {
  AO_REQUIRE(format == AO_OPTIM_Q8_SIGNED || format == AO_OPTIM_Q4_SIGNED || format == AO_OPTIM_FP8 || format == AO_OPTIM_PLAIN,
             "%s: format must be the first moment's (AO_OPTIM_Q8_SIGNED, AO_OPTIM_Q4_SIGNED, AO_OPTIM_FP8) or AO_OPTIM_PLAIN, got %d", __func__,
             format);
  const int kind = kind_of(format);
  if (kind == K_PLAIN) {
    AO_REQUIRE(n >= 0 && n < (1ll << 40), "%s: n=%lld must be in [0, 2^40)", __func__, (long long)n);
  } else if (int rc = check_quantized(__func__, n, block_size, kind)) {
    return rc;
  }
  AO_REQUIRE(max_workgroups >= 0, "%s: max_workgroups=%d must not be negative", __func__, max_workgroups);
  AO_REQUIRE(!sr || bf16, "%s: stochastic rounding is for bf16 parameters", __func__);
  AO_REQUIRE(step >= 0 && param_index >= 0, "%s: step and param_index must not be negative", __func__);
  AO_REQUIRE_PTR(scalars);
  if (n == 0) return AO_OK;
  AO_REQUIRE_PTR(p);
  AO_REQUIRE_PTR(grad);
  AO_REQUIRE(aligned_to(p, 16) && aligned_to(grad, 16), "%s: p and grad must be 16-byte aligned", __func__);
  StepArgs a{};
  a.p = p;
  a.g = grad;
  a.m = Moment{m_codes, m_scale, m_qmap};
  a.v = Moment{v_codes, v_scale, v_qmap};
  a.vmax = Moment{vmax_codes, vmax_scale, vmax_qmap};
  if (int rc = check_moment(__func__, "m", a.m, kind)) return rc;
  if (int rc = check_moment(__func__, "v", a.v, kind)) return rc;
  a.has_vmax = vmax_codes != nullptr;
  if (a.has_vmax)
    if (int rc = check_moment(__func__, "vmax", a.vmax, kind)) return rc;
  a.n = n;
  a.tiles = tiles_of(n);
  a.lb = kind == K_PLAIN ? 4 : log2_block(block_size);
  a.s = *scalars;
  a.is_adamw = is_adamw != 0;
  a.sr = sr != 0;
  a.k0 = (uint32_t)((uint64_t)seed & 0xffffffffu);
  a.k1 = (uint32_t)((uint64_t)seed >> 32);
  a.step = (uint32_t)((uint64_t)step & 0xffffffffu);
  a.param = (uint32_t)((uint64_t)param_index & 0xffffffffu);
  dispatch<StepLaunch>(kind, bf16 != 0, a, dim3((unsigned)grid_of(a.tiles, max_workgroups)), (hipStream_t)stream);
  AO_LAUNCH_CHECK("optim_adam_kernel launch");
  return AO_OK;
}
