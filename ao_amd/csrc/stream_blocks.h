// Device building blocks the weight-streaming linears share: the 128-k MFMA step of 8-bit (and MX 4-bit) operands, parking a wave's
// accumulator tile for the cross-wave split-K meeting in LDS, and the workgroup-wide per-row activation cast into LDS.  The K loops that
// feed them (rings, chunks, slabs) and the epilogues behind them stay with the kernels.
// Not here: the sums of the meeting (the waves' parked tiles added in wave order: reproducible).  As functions -- by pointer, by
// reference to the LDS array, through a callable -- they changed the code of the product kernels around them (dec8_kernel's epilogue
// loop grew by two to three instructions, the MX stream kernels went from 36 .. 48 to 70 VGPRs, mx_grouped_kernel gained 12 .. 48), so
// each kernel keeps its three to nine lines.
#pragma once
#include "common.h"
#include "quant_math.h"

namespace ao {

// 8 + 8 dwords of a lane -> the scaled MFMA's 256-bit operand
__device__ __forceinline__ i32x8 pack_k128(u32x4 lo, u32x4 hi) {
  return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}
// the scaled MFMA of mfma8_k128 on operands a kernel packed itself (pack_k128) because it keeps them across steps or tiles
template <int FMT = 0>
__device__ __forceinline__ f32x4 mfma8_k128_packed(i32x8 af, i32x8 bf, f32x4 acc, int sa = 127, int sb = 127) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bf, acc, FMT, FMT, 0, sa, 0, sb);
}
// One 128-k step of a 16 x 16 tile, the new accumulator returned.  Operand layout (probed on gfx950, tools/probe_mfma_scale.hip): lane
// l holds row / column l & 15; 8-bit elements: lane group kq = l >> 4 holds k = 16 kq .. +15 in a0 / b0 and 64 + 16 kq .. +15 in
// a1 / b1; e2m1 (FMT 4): k = 32 kq .. +31 in a0 / b0, a1 / b1 unused.
//   INT8: two v_mfma_i32_16x16x64_i8, acc holds int32 bit patterns.
//   else: one v_mfma_scale_f32_16x16x128_f8f6f4 on elements of MFMA format code FMT (cbsz / blgp: 0 e4m3, 4 e2m1); sa / sb are the
//         lane's E8M0 scale bytes of 32-k block kq (MX), 127 = 2^0 for operands without block scales.
// (Operands by value: through references the register allocation of dyn8_kernel's fp8 loop came out differently.)
template <bool INT8, int FMT = 0>
__device__ __forceinline__ f32x4 mfma8_k128(u32x4 a0, u32x4 a1, u32x4 b0, u32x4 b1, f32x4 acc, int sa = 127, int sb = 127) {
  if constexpr (INT8) {
    i32x4 c = __builtin_bit_cast(i32x4, acc);
    c = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a0), __builtin_bit_cast(i32x4, b0), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a1), __builtin_bit_cast(i32x4, b1), c, 0, 0, 0);
    return __builtin_bit_cast(f32x4, c);
  } else {
    return mfma8_k128_packed<FMT>(pack_k128(a0, a1), pack_k128(b0, b1), acc, sa, sb);
  }
}

// A wave parks its accumulator tile for the meeting as [row 16][col 16] floats (D layout: lane (col nl, group kq) holds rows 4 kq + {0..3})
__device__ __forceinline__ void park_tile(float* tile, int kq, int nl, f32x4 acc) {
  float* r = tile + (kq * 4) * 16 + nl;
  r[0] = acc.x; r[16] = acc.y; r[32] = acc.z; r[48] = acc.w;
}

// The per-row cast of an M x K bf16 activation (M <= 16) into codes in LDS by the whole workgroup, with the arithmetic of the
// stand-alone casts (quant_math.h), in two passes over the L2-resident rows: row amax -> rs[row] (wmax: [waves][16] scratch), then
// codes -> xq, rows `stride` bytes apart.  LDS_ONLY: the two barriers in between are lds_barrier() (a kernel with weight loads in
// flight), else __syncthreads().  The caller puts its own barrier between the codes and their readers.
template <bool INT8, bool LDS_ONLY>
__device__ __forceinline__ void cast_rows_to_lds(const uint16_t* x, int M, int K, char* xq, int stride, float* wmax, float* rs) {
  const int tid = threadIdx.x, lane = tid & 63, nthreads = blockDim.x, nwaves = nthreads >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  auto barrier = [] {
    if constexpr (LDS_ONLY) lds_barrier();
    else __syncthreads();
  };
  const int nvec = K >> 3;  // 8 bf16 per 16 B
  for (int r = 0; r < M; ++r) {
    const u32x4* xr = reinterpret_cast<const u32x4*>(x + (size_t)r * K);
    float m = 0.f;
    bool has_nan = false;
    for (int i = tid; i < nvec; i += nthreads) m = fmaxf(m, amax8(xr[i], has_nan));
    if (has_nan) m = INFINITY;  // (NaN rows are outside the contract, as in the stand-alone cast)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) wmax[wave * 16 + r] = m;
  }
  barrier();
  if (tid < M) {
    float m = 0.f;
    for (int w = 0; w < nwaves; ++w) m = fmaxf(m, wmax[w * 16 + tid]);
    rs[tid] = INT8 ? int8_row_scale(m) : fp8_row_scale(m);
  }
  barrier();
  for (int r = 0; r < M; ++r) {
    const u32x4* xr = reinterpret_cast<const u32x4*>(x + (size_t)r * K);
    const float s = rs[r];
    const float inv = 1.0f / s;
    for (int i = tid; i < nvec; i += nthreads)
      *reinterpret_cast<u32x2*>(xq + r * stride + i * 8) = INT8 ? int8_quant8(xr[i], inv) : fp8_quant8(xr[i], s);
  }
}

}  // namespace ao
