// The frame of the weight-gradient GEMMs (mx_wgrad_kernels.hip, fp8_grouped_train_kernels.hip, fp8_block_train_kernels.hip): 2-D x 2-D
// grouped GEMMs on e4m3 codes stored with the tokens contiguous ([N][M] and [K][M]),
//   out[e][n][k] = bf16( sum over the tokens m of group e = [offs[e-1], offs[e]) of g[n][m] x[k][m], scaled as the recipe says ).
// Grid (tiles of K, tiles of N, E), 128 x 128 output tiles, four waves of 64 x 64, both operands staged in LDS by buffer_load ... lds
// (16 bytes a lane), two stages; rows past N / K and tokens past M read as zero through the buffer's range check.  The k steps walk the
// GLOBAL 128-token grid from start / 128 to ceil(end / 128), so every 16-byte load and every scale index is aligned as in a dense GEMM
// whatever the offsets are.  A step that reaches outside [start, end) (only a group's first and last can) zeroes the g code bytes of the
// foreign tokens in registers, behind a wave-uniform branch.  (Only g is masked: a foreign token's x code meets a zero.  Non-finite codes
// of a neighbour group inside a shared 128-token step therefore still reach this group as NaN, as 0 x NaN.)  An empty group runs no step
// and stores zeros; no offs: one group of every token, a dense linear's weight gradient.  No split along the tokens: a launch is
// reproducible.
//
// A recipe differs only in where its scales enter, which its POLICY says (wgrad_tile below lists the three hooks):
//   MXFP8     E8M0 bytes inside the MFMA, prefetched per step                              (mx_wgrad_kernels.hip)
//   rowwise   two reciprocal vectors per expert in the epilogue, nothing per step          (fp8_grouped_train_kernels.hip)
//   blockwise fp8_block_acc per step on a zero-based product, reciprocals prefetched       (fp8_block_train_kernels.hip)
#pragma once
#include <string>

#include "common.h"

namespace ao {
namespace wgrad_frame {

// Stage layout (that of mx_linear_tile_kernel): g then x, 128 rows each, 128 bytes (one k step of tokens) a row, 16-byte pieces swizzled by
// row so that the 16 lanes of a fragment read hit different banks: piece c of row r sits at slot r * 8 + (c ^ (r % 8)).
constexpr int kOpBytes = 128 * 128;
constexpr int kStage = 2 * kOpBytes;
constexpr size_t kLdsBytes = 2 * kStage;  // the frame's dynamic LDS: two stages

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, char* lds, uint32_t voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds, 16, voff, 0, 0, 0);
}

__device__ __forceinline__ void wgrad_issue(__amdgpu_buffer_rsrc_t rg, __amdgpu_buffer_rsrc_t rx, char* stage, int n0, int k0, int step, int M,
                                            int N, int K, int wave, int lane) {
  constexpr int kInstr = kOpBytes / 1024;  // 1 KiB per wave instruction
#pragma unroll
  for (int i = wave; i < 2 * kInstr; i += 4) {
    const bool isx = i >= kInstr;
    const int j = isx ? i - kInstr : i;
    const int slot = j * 64 + lane;
    const int r = slot >> 3, c = (slot & 7) ^ (r & 7);
    const int tok = step * 128 + c * 16;
    const int grow = (isx ? k0 : n0) + r;
    const uint32_t voff = (tok < M && grow < (isx ? K : N)) ? (uint32_t)grow * (uint32_t)M + (uint32_t)tok : 0xFFFFFFF0u;
    dma16(isx ? rx : rg, stage + (isx ? kOpBytes : 0) + j * 1024, voff);
  }
}

__device__ __forceinline__ void wgrad_frag(const char* op, int r, int kq, u32x4& v0, u32x4& v1) {
  v0 = *reinterpret_cast<const u32x4*>(op + (r * 8 + (kq ^ (r & 7))) * 16);
  v1 = *reinterpret_cast<const u32x4*>(op + (r * 8 + ((kq + 4) ^ (r & 7))) * 16);
}

// 0xFF in the bytes j < n of a dword
__device__ __forceinline__ uint32_t bytes_below(int n) { return n <= 0 ? 0u : (n >= 4 ? 0xFFFFFFFFu : (1u << (8 * n)) - 1u); }

// 0xFF in the bytes of 16 consecutive tokens from `t0` on that lie in [start, end)
__device__ __forceinline__ u32x4 token_mask(int t0, int start, int end) {
  u32x4 m;
#pragma unroll
  for (int d = 0; d < 4; ++d) m[d] = bytes_below(end - t0 - 4 * d) & ~bytes_below(start - t0 - 4 * d);
  return m;
}

// Where a lane stands in its tile.  Operand fragment i reads row wn + 16 i + l16 of g (j: wk + 16 j + l16 of x); the accumulator
// acc[i][j][r] is out[nrow + 16 i + r][kcol + 16 j].
struct Lane {
  int l16, kq;  // lane % 16, lane / 16
  int n0, k0;   // the tile's first row of g and of x
  int wn, wk;   // the wave's 64 x 64 quarter of it
  __device__ __forceinline__ int nrow() const { return n0 + wn + 4 * kq; }
  __device__ __forceinline__ int kcol() const { return k0 + wk + l16; }
};

// The walk over a lane's [n][k] that stores bf16(value(i, j, r, n, k)); EDGES false: N and K are multiples of 128, nothing to check.
template <bool EDGES, class F>
__device__ __forceinline__ void wgrad_store(uint16_t* out, const Lane& t, int N, int K, F value) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = t.kcol() + 16 * j;
    if (EDGES && k >= K) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = t.nrow() + 16 * i + r;
        if (!EDGES || n < N) out[(size_t)n * K + k] = f32_to_bf16_bits(value(i, j, r, n, k));
      }
  }
}

// One workgroup's tile of one group.  Args: g, x (the codes), offs (null: one group [0, M)), out (bf16 [E][N][K]), M, N, K and what the
// policy reads.  Policy:
//   Policy(args, lane, e)                          what the lane keeps for the whole tile (its scale pointers)
//   struct Scales; load(step, Scales&)             the lane's scales of one k step into registers (rowwise: none)
//   mac(acc, g0, g1, x0, x1, Scales, i, j)         one 16 x 16 x 128 multiply-accumulate of fragments i and j, the new accumulator returned
//   store(out_e, acc, lane)                        the tile's epilogue, through wgrad_store
template <class Policy, class Args>
__device__ __forceinline__ void wgrad_tile(const Args& p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // A function is optimised on its own before it is inlined into its kernel, and only the kernel carries __launch_bounds__(256): without
  // the bound stated here wave could be up to 15, wgrad_issue's loop over `i = wave; i < 32; i += 4` has no fixed trip count, and the
  // kernel comes out with guarded copies of it, more registers and a slower loop.  (An assumption about a call is discarded: the local.)
  const unsigned tid = threadIdx.x;
  __builtin_assume(tid < 256u);
  const int lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
  const int e = blockIdx.z;
  const Lane t{lane & 15, kq, (int)blockIdx.y * 128, (int)blockIdx.x * 128, (wave >> 1) * 64, (wave & 1) * 64};
  // the group's tokens, clamped to the matrix; a range that runs backwards is an empty group
  const int start = p.offs != nullptr ? min(max(e > 0 ? p.offs[e - 1] : 0, 0), p.M) : 0;
  const int end = p.offs != nullptr ? min(max(p.offs[e], 0), p.M) : p.M;
  const int s0 = start >> 7, s1 = end > start ? (end + 127) >> 7 : s0;
  // rows past the matrix fall outside the buffer's range and read as zero
  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)p.g, 0, p.N * p.M, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.K * p.M, 0x00020000);
  const Policy pol(p, t, e);
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  typename Policy::Scales sc;
  if (s0 < s1) {
    pol.load(s0, sc);
    wgrad_issue(rg, rx, smem + (s0 & 1) * kStage, t.n0, t.k0, s0, p.M, p.N, p.K, wave, lane);
  }
  for (int step = s0; step < s1; ++step) {
    char* cur = smem + (step & 1) * kStage;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage `step` has landed for every wave; every wave is done with the other stage
    typename Policy::Scales next;
    if (step + 1 < s1) {
      wgrad_issue(rg, rx, smem + ((step + 1) & 1) * kStage, t.n0, t.k0, step + 1, p.M, p.N, p.K, wave, lane);
      pol.load(step + 1, next);
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
    for (int j = 0; j < 4; ++j) wgrad_frag(cur + kOpBytes, t.wk + 16 * j + t.l16, kq, xf0[j], xf1[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 g0, g1;
      wgrad_frag(cur, t.wn + 16 * i + t.l16, kq, g0, g1);
      if (edge) {
        g0 &= mk0;
        g1 &= mk1;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = pol.mac(acc[i][j], g0, g1, xf0[j], xf1[j], sc, i, j);
    }
    if (step + 1 < s1) sc = next;
  }
  pol.store(p.out + (size_t)e * p.N * p.K, acc, t);
}

// ---- the host side of the entries -----------------------------------------------------------------------------------------------------------
// What an entry requires: the name it gives the token count, the multiples of the token count and of N and K, and whether offs may be
// null (then E must be 1: one group of every token).
struct Entry {
  const char* fn;
  const char* m_name;
  int m_mult, nk_mult;
  bool offs_optional;
};

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The checks every entry makes, in the order a caller meets them: the shape, the grid's and the 32-bit indices' limits, out, then -- unless
// there are no tokens, when out is zeroed and *launch is false -- the codes and offs.  The scales are the entry's to check.
inline int check_entry(const Entry& c, const void* g_t, const void* x_t, const int32_t* offs, uint16_t* out, int64_t M, int64_t N, int64_t K,
                       int64_t E, hipStream_t st, bool* launch) {
  const char* fn = c.fn;
  *launch = false;
  AO_REQUIRE(M >= 0 && N > 0 && K > 0 && E > 0, "%s: bad shape %s=%lld N=%lld K=%lld E=%lld", fn, c.m_name, (long long)M, (long long)N,
             (long long)K, (long long)E);
  const struct { const char* name; int64_t v; int mult; } dims[3] = {{c.m_name, M, c.m_mult}, {"N", N, c.nk_mult}, {"K", K, c.nk_mult}};
  for (const auto& d : dims)
    AO_REQUIRE(d.v % d.mult == 0, "%s: %s=%lld must be a multiple of %d (the tokens, N and K must be multiples of %d, %d and %d)", fn, d.name,
               (long long)d.v, d.mult, c.m_mult, c.nk_mult, c.nk_mult);
  AO_REQUIRE(E < 65536 && (N + 127) / 128 < 65536, "%s: E=%lld must be below 65536 and N=%lld below 65536 tiles of 128 (the grid's z and y extents)",
             fn, (long long)E, (long long)N);
  if (c.offs_optional)
    AO_REQUIRE(offs != nullptr || E == 1, "%s: without offs there is one group of every token, got E=%lld", fn, (long long)E);
  AO_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31) && N * M < (1ll << 31) && K * M < (1ll << 31),
             "%s: %s=%lld N=%lld K=%lld: the sizes and both operands' byte counts must be below 2^31", fn, c.m_name, (long long)M, (long long)N,
             (long long)K);
  AO_REQUIRE_PTR_FN(fn, out);
  if (M == 0) {
    const hipError_t rc = hipMemsetAsync(out, 0, (size_t)E * N * K * sizeof(uint16_t), st);
    return rc != hipSuccess ? hip_failed(rc, "hipMemsetAsync(weight gradient of no tokens)") : AO_OK;
  }
  AO_REQUIRE_PTR_FN(fn, g_t);
  AO_REQUIRE_PTR_FN(fn, x_t);
  if (!c.offs_optional) AO_REQUIRE_PTR_FN(fn, offs);
  AO_REQUIRE(aligned16(g_t) && aligned16(x_t), "%s: the codes must be 16-byte aligned", fn);
  *launch = true;
  return AO_OK;
}

template <class Args>
int launch_frame(void (*kernel)(Args), const char* kernel_name, const Args& args, int64_t N, int64_t K, int64_t E, hipStream_t st) {
  const std::string name(kernel_name);  // an error says which of the two calls failed
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), kLdsBytes, ("hipFuncSetAttribute(" + name + ")").c_str())) return rc;
  ao::launch(kernel, dim3((unsigned)((K + 127) / 128), (unsigned)((N + 127) / 128), (unsigned)E), dim3(256), kLdsBytes, st, args);
  AO_LAUNCH_CHECK((name + " launch").c_str());
  return AO_OK;
}

}  // namespace wgrad_frame
}  // namespace ao
