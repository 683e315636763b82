// The weight gradient of the MXFP8 MoE grouped GEMM for gfx950: a 2-D x 2-D grouped GEMM whose contraction runs over each expert's tokens.
//
// Replaces the GEMM of _compute_wgrad (torchao/prototype/moe_training/mxfp8_grouped_mm.py:712-796: torch._scaled_grouped_mm on the 32 x 1
// casts of grad_output and input_act with K-group blocked scales), with the numerics of _emulated_mxfp8_scaled_grouped_mm_2d_2d
// (:1026-1057): both operands dequantised per 32-token block, fp32 accumulation, one rounding to bf16:
//   out[e][n][k] = bf16( sum_{m in [offs[e-1], offs[e])} dq(g)[m][n] dq(x)[m][k] ),  dq = element 2^(scale - 127).
// The operands are what ao_mxfp8_quantize_colwise writes: codes transposed ([N][M_total] and [K][M_total], tokens contiguous) and one scale per
// 32 tokens on the GLOBAL block grid ([M_total/32][rows]), so a row of codes is a row of a dense MX operand whose contraction index is the token
// -- mx_linear_tile_kernel<e4m3> (mx_linear_kernels.hip) with the scales transposed and the k range cut per expert.
//
// mx_wgrad_kernel: grid (tiles of K, tiles of N, E), 128 x 128 output tiles, four waves of 64 x 64, both operands staged in LDS by
// buffer_load ... lds (16 bytes a lane), two stages; rows past N / K and tokens past M_total read as zero through the buffer's range check.
// The k steps walk the global 128-token grid from start / 128 to ceil(end / 128), so every 16-byte load and every scale index is aligned as
// in the dense kernel whatever the offsets are.  A step that reaches outside [start, end) (only a group's first and last can) zeroes the g
// code bytes of the foreign tokens in registers, behind a wave-uniform branch: a 32-token block that straddles a boundary lends its scale to
// both groups and each sums its own tokens.  (Only g is masked: a foreign token's x code meets a zero.  Non-finite codes or scales of a
// neighbour group inside a shared 128-token step therefore still reach this group as NaN, as 0 x NaN.)
// An empty group runs no step and stores zeros.
#include "common.h"
#include "stream_blocks.h"
#include "wgrad_stage.h"

namespace ao {
namespace {

using namespace wgrad_stage;  // the stage layout, wgrad_issue, wgrad_frag, token_mask

struct WgradArgs {
  const uint8_t* g;        // e4m3 [N][M]
  const uint8_t* g_scale;  // e8m0 [M/32][N]
  const uint8_t* x;        // e4m3 [K][M]
  const uint8_t* x_scale;  // e8m0 [M/32][K]
  const int32_t* offs;     // [E] cumulative ends; null: one group [0, M)
  uint16_t* out;           // bf16 [E][N][K]
  int M, N, K;
};

// the lane's scale byte of row `row`, 32-token block `blk`: the 16 lanes of a fragment read consecutive bytes
__device__ __forceinline__ int wgrad_scale(const uint8_t* scales, int row, int rows, int blk, int mb) {
  return (row < rows && blk < mb) ? (int)scales[(size_t)blk * rows + row] : 127;
}

__global__ __launch_bounds__(256) void mx_wgrad_kernel(WgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4;
  const int e = blockIdx.z;
  const int n0 = blockIdx.y * 128, k0 = blockIdx.x * 128;
  const int wn = (wave >> 1) * 64, wk = (wave & 1) * 64;
  const int mb = p.M >> 5;
  // the group's tokens, clamped to the matrix; a range that runs backwards is an empty group
  // (no offs: one group of every token, the dense linear's weight gradient)
  const int start = p.offs != nullptr ? min(max(e > 0 ? p.offs[e - 1] : 0, 0), p.M) : 0;
  const int end = p.offs != nullptr ? min(max(p.offs[e], 0), p.M) : p.M;
  const int s0 = start >> 7, s1 = end > start ? (end + 127) >> 7 : s0;
  // rows past the matrix fall outside the buffer's range and read as zero
  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)p.g, 0, p.N * p.M, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.K * p.M, 0x00020000);
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int sg[4], sx[4];
  if (s0 < s1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sg[i] = wgrad_scale(p.g_scale, n0 + wn + 16 * i + (lane & 15), p.N, s0 * 4 + kq, mb);
      sx[i] = wgrad_scale(p.x_scale, k0 + wk + 16 * i + (lane & 15), p.K, s0 * 4 + kq, mb);
    }
    wgrad_issue(rg, rx, smem + (s0 & 1) * kStage, n0, k0, s0, p.M, p.N, p.K, wave, lane);
  }
  for (int step = s0; step < s1; ++step) {
    char* cur = smem + (step & 1) * kStage;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage `step` has landed for every wave; every wave is done with the other stage
    int ng[4], nx[4];
    if (step + 1 < s1) {
      wgrad_issue(rg, rx, smem + ((step + 1) & 1) * kStage, n0, k0, step + 1, p.M, p.N, p.K, wave, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ng[i] = wgrad_scale(p.g_scale, n0 + wn + 16 * i + (lane & 15), p.N, (step + 1) * 4 + kq, mb);
        nx[i] = wgrad_scale(p.x_scale, k0 + wk + 16 * i + (lane & 15), p.K, (step + 1) * 4 + kq, mb);
      }
    }
    // a step that reaches outside the group: the lane's two 16-token pieces keep the group's own tokens only
    const bool edge = step * 128 < start || step * 128 + 128 > end;  // wave-uniform
    u32x4 mk0, mk1;
    if (edge) {
      mk0 = token_mask(step * 128 + 16 * kq, start, end);
      mk1 = token_mask(step * 128 + 64 + 16 * kq, start, end);
    }
    u32x4 xf0[4], xf1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wgrad_frag(cur + kOpBytes, wk + 16 * j + (lane & 15), kq, xf0[j], xf1[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 g0, g1;
      wgrad_frag(cur, wn + 16 * i + (lane & 15), kq, g0, g1);
      if (edge) {
        g0 &= mk0;
        g1 &= mk1;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma8_k128<false, AO_MX_FMT_E4M3>(g0, g1, xf0[j], xf1[j], acc[i][j], sg[i], sx[j]);
    }
    if (step + 1 < s1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sg[i] = ng[i];
        sx[i] = nx[i];
      }
    }
  }
  uint16_t* out = p.out + (size_t)e * p.N * p.K;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = k0 + wk + 16 * j + (lane & 15);
    if (k >= p.K) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + 16 * i + 4 * kq + r;
        if (n < p.N) out[(size_t)n * p.K + k] = f32_to_bf16_bits(acc[i][j][r]);
      }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace
}  // namespace ao

using namespace ao;

namespace {
// (AO_REQUIRE_PTR names the enclosing function: here the entry's name is `fn`)
#define WGRAD_REQUIRE_PTR(p)                                    \
  do {                                                          \
    if ((p) == nullptr) {                                       \
      ::ao::set_error("%s: null pointer argument '%s'", fn, #p); \
      return AO_ERR_NULL_POINTER;                               \
    }                                                           \
  } while (0)

// dense: one group [0, M_total) and no offs tensor (E == 1)
int wgrad(const char* fn, const uint8_t* g_t, const uint8_t* g_scale, const uint8_t* x_t, const uint8_t* x_scale, const int32_t* offs, uint16_t* out,
          int64_t M_total, int64_t N, int64_t K, int64_t E, bool dense, void* stream) {
  AO_REQUIRE(M_total >= 0 && N > 0 && K > 0 && E > 0, "%s: bad shape M_total=%lld N=%lld K=%lld E=%lld", fn, (long long)M_total,
             (long long)N, (long long)K, (long long)E);
  AO_REQUIRE(M_total % 32 == 0, "%s: M_total=%lld must be a multiple of 32 (one scale per 32 tokens)", fn, (long long)M_total);
  AO_REQUIRE(N % 16 == 0, "%s: N=%lld must be a multiple of 16", fn, (long long)N);
  AO_REQUIRE(K % 16 == 0, "%s: K=%lld must be a multiple of 16", fn, (long long)K);
  AO_REQUIRE(E < 65536, "%s: E=%lld must be below 65536 (the grid's z extent)", fn, (long long)E);
  AO_REQUIRE(M_total < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31) && N * M_total < (1ll << 31) && K * M_total < (1ll << 31),
             "%s: M_total=%lld N=%lld K=%lld: the sizes and both operands' byte counts must be below 2^31", fn, (long long)M_total,
             (long long)N, (long long)K);
  WGRAD_REQUIRE_PTR(out);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (M_total == 0) {
    const hipError_t rc = hipMemsetAsync(out, 0, (size_t)E * N * K * sizeof(uint16_t), st);
    if (rc != hipSuccess) return hip_failed(rc, "hipMemsetAsync(mx_wgrad)");
    return AO_OK;
  }
  WGRAD_REQUIRE_PTR(g_t);
  WGRAD_REQUIRE_PTR(g_scale);
  WGRAD_REQUIRE_PTR(x_t);
  WGRAD_REQUIRE_PTR(x_scale);
  if (!dense) WGRAD_REQUIRE_PTR(offs);
  AO_REQUIRE(aligned16(g_t) && aligned16(x_t), "%s: the codes must be 16-byte aligned", fn);
  constexpr size_t smem = 2 * kStage;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(mx_wgrad_kernel), smem, "hipFuncSetAttribute(mx_wgrad_kernel)")) return rc;
  const WgradArgs args{g_t, g_scale, x_t, x_scale, dense ? nullptr : offs, out, (int)M_total, (int)N, (int)K};
  ao::launch(mx_wgrad_kernel, dim3((unsigned)((K + 127) / 128), (unsigned)((N + 127) / 128), (unsigned)E), dim3(256), smem, st, args);
  AO_LAUNCH_CHECK("mx_wgrad_kernel launch");
  return AO_OK;
}
#undef WGRAD_REQUIRE_PTR
}  // namespace

extern "C" int ao_mxfp8_grouped_mm_wgrad(const uint8_t* g_t, const uint8_t* g_scale, const uint8_t* x_t, const uint8_t* x_scale,
                                         const int32_t* offs, uint16_t* out, int64_t M_total, int64_t N, int64_t K, int64_t E, void* stream) {
  return wgrad(__func__, g_t, g_scale, x_t, x_scale, offs, out, M_total, N, K, E, false, stream);
}

extern "C" int ao_mxfp8_mm_wgrad(const uint8_t* g_t, const uint8_t* g_scale, const uint8_t* x_t, const uint8_t* x_scale, uint16_t* out, int64_t M,
                                 int64_t N, int64_t K, void* stream) {
  return wgrad(__func__, g_t, g_scale, x_t, x_scale, nullptr, out, M, N, K, 1, true, stream);
}
