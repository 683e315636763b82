// Shared host/device helpers for the gfx950 low-bit kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/ao_mi355.h"

namespace ao {

// ---- host side: error plumbing (thread-local message, never exit()) --------
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int hip_failed(hipError_t e, const char* what);  // sets message, returns AO_ERR_HIP

// The A/B overrides of ao_int4_set_tuning (int4_kernels.hip; default-constructed: the product dispatch): waves per workgroup of the
// per-tile kernel, the int4 mm's forced form (int4_forced_route), and the fp8-act x int4 forms of modes 961 - 974.
struct Int4Force {
  int wpb = 0, mode = 0;
  int fp8_mt = 0;        // m-tiles per workgroup forced (1, 2, 4; 0 = by M)
  bool fp8_nt1 = false;  // one n-tile per workgroup
};
const Int4Force& int4_force();  // the calling thread's

// opt a kernel into > 48 KiB of dynamic LDS on the current device (once per kernel and device; runtime.hip)
int ensure_dynamic_lds(const void* kernel, size_t bytes, const char* what);

// whether p sits on a multiple of a, a power of two (null does: the entries check their required pointers on their own)
inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

#define AO_REQUIRE(cond, ...)                \
  do {                                       \
    if (!(cond)) {                           \
      ::ao::set_error(__VA_ARGS__);          \
      return AO_ERR_INVALID_ARGUMENT;        \
    }                                        \
  } while (0)

// (fn: the entry's name, where a helper shared by several entries makes the check)
#define AO_REQUIRE_PTR_FN(fn, p)                                 \
  do {                                                           \
    if ((p) == nullptr) {                                        \
      ::ao::set_error("%s: null pointer argument '%s'", fn, #p); \
      return AO_ERR_NULL_POINTER;                                \
    }                                                            \
  } while (0)
#define AO_REQUIRE_PTR(p) AO_REQUIRE_PTR_FN(__func__, p)

#define AO_LAUNCH_CHECK(what)                          \
  do {                                                 \
    hipError_t e__ = hipGetLastError();                \
    if (e__ != hipSuccess) return ::ao::hip_failed(e__, what); \
  } while (0)

// ---- launch helper ---------------------------------------------------------
// While profiling is enabled (ao_prof_enable) every launch is bracketed by HIP
// extension events that timestamp the dispatch itself (kernel begin/end, no
// launch gaps) -- what bench.py uses for the live roofline numbers.
bool prof_next_events(hipEvent_t* start, hipEvent_t* stop);

template <typename K, typename... Args>
inline void launch(K kernel, dim3 grid, dim3 block, size_t smem, hipStream_t stream, Args... args) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (prof_next_events(&e0, &e1)) {
    hipExtLaunchKernelGGL(kernel, grid, block, (unsigned)smem, stream, e0, e1, 0, args...);
  } else {
    hipLaunchKernelGGL(kernel, grid, block, (unsigned)smem, stream, args...);
  }
}

// ---- host side: the two launch ladders -----------------------------------------
// A group size of {32, 64, 128, 256} (the entry has checked the set) as a compile-time G: f(std::integral_constant<int, G>{}).
template <typename F>
inline auto with_group_size(int group_size, F&& f) {
  switch (group_size) {
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    case 128: return f(std::integral_constant<int, 128>{});
    default: return f(std::integral_constant<int, 256>{});
  }
}

constexpr int kRowThreads = 256;  // the workgroup of the kernels that own a row: four waves (block_max / block_sum below)

// The register depth of a row kernel: NV = 1, 2, 4 or 8 16-byte vectors a thread, the least that holds a row of `row_elems` 2-byte elements
// in the registers of kRowThreads threads: f(std::integral_constant<int, NV>{}).  False, and f not called, where the row is longer (K > 16384).
template <typename F>
inline bool with_row_depth(int64_t row_elems, F&& f) {
  const int64_t per_thread = ((row_elems >> 3) + kRowThreads - 1) / kRowThreads;
  if (per_thread <= 1) f(std::integral_constant<int, 1>{});
  else if (per_thread <= 2) f(std::integral_constant<int, 2>{});
  else if (per_thread <= 4) f(std::integral_constant<int, 4>{});
  else if (per_thread <= 8) f(std::integral_constant<int, 8>{});
  else return false;
  return true;
}

// the shape rules of the entries that take M rows of K elements, K a multiple of `mult`
inline int check_rows(const char* fn, int64_t M, int64_t K, int64_t mult) {
  AO_REQUIRE(M >= 0 && K > 0, "%s: bad shape M=%lld K=%lld", fn, (long long)M, (long long)K);
  AO_REQUIRE(K % mult == 0, "%s: K=%lld must be a multiple of %lld", fn, (long long)K, (long long)mult);
  AO_REQUIRE(M < (1ll << 31), "%s: M=%lld too large", fn, (long long)M);
  return AO_OK;
}

// ---- device side -----------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kWave = 64;  // gfx950 wavefront

// workgroup barrier that orders LDS traffic only: __syncthreads() carries a workgroup-scope release fence, which on gfx9 means
// s_waitcnt vmcnt(0) -- it would drain the weight loads a streaming kernel keeps in flight across its barriers
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ float bits_to_f32(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t f32_to_bits(float f) { return __float_as_uint(f); }

// bf16 bit pattern (in the low 16 bits) -> fp32
__device__ __forceinline__ float bf16_lo_to_f32(uint32_t packed) { return bits_to_f32(packed << 16); }
__device__ __forceinline__ float bf16_hi_to_f32(uint32_t packed) { return bits_to_f32(packed & 0xffff0000u); }

// two fp32 -> packed bf16 pair, round-to-nearest-even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  f32x2 v = {lo, hi};
  bf16x2 r = __builtin_convertvector(v, bf16x2);
  return __builtin_bit_cast(uint32_t, r);
}

// fp32 -> fp32 holding the nearest bf16 value (RNE), i.e. torch's ".to(bf16)"
__device__ __forceinline__ float round_bf16(float f) {
  __bf16 b = (__bf16)f;
  return (float)b;
}

// a * b rounded to fp32 on its own.  The int8 epilogue adds the bias to the rounded product (int8_tensor.py:315-359: two tensor ops),
// so the multiply and that add must not be contracted into one v_fma_f32.
__device__ __forceinline__ float mul_f32_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

__device__ __forceinline__ uint16_t f32_to_bf16_bits(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(uint16_t, b);
}

// max over the 16 lanes of a DPP row, in every one of them
__device__ __forceinline__ float row16_max(float m) {
  auto dpp = [](float v, auto ctrl) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xF, 0xF, true));
  };
  m = fmaxf(m, dpp(m, std::integral_constant<int, 0xB1>{}));   // quad_perm [1,0,3,2]
  m = fmaxf(m, dpp(m, std::integral_constant<int, 0x4E>{}));   // quad_perm [2,3,0,1]
  m = fmaxf(m, dpp(m, std::integral_constant<int, 0x141>{}));  // row_half_mirror
  m = fmaxf(m, dpp(m, std::integral_constant<int, 0x140>{}));  // row_mirror
  return m;
}

// max over the 64 lanes without LDS traffic: DPP within rows of 16, then the four row results through SGPRs
__device__ __forceinline__ float wave_max(float m) {
  m = row16_max(m);
  const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, m), 0));
  const float b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, m), 16));
  const float c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, m), 32));
  const float d = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, m), 48));
  return fmaxf(fmaxf(a, b), fmaxf(c, d));
}

// max / sum over the kRowThreads threads of a workgroup, in every one of them: the wave's own reduction, then the four waves meet in `red`
// (4 floats of LDS, free again on return).  max is exact, and the sum's order is fixed, so every launch gives the same bytes.
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return v;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);  // every lane ends with the same bits: a + b and b + a round alike
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}

}  // namespace ao
