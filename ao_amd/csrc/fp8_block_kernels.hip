// Blockwise float8 (e4m3fn) linears for gfx950: 1 x 128 activation blocks, 128 x 128 weight blocks, fp32 scales.
//
// The third granularity of Float8DynamicActivationFloat8WeightConfig, [PerBlock([1, 128]), PerBlock([128, 128])] (quant_api.py:1112-1297;
// the layout of the DeepSeek-V3 / Qwen3 FP8 checkpoints: weight_scale_inv is the [N/128][K/128] scale).  Replaces the casts of
// Float8Tensor.from_hp with kernel_choice "torch" (quantize_/workflows/float8/float8_tensor.py:233-242, quant_primitives.py:2173-2212,
// :2271-2287) and the Triton GEMM blockwise_fp8_gemm (quantize_/workflows/float8/kernels.py:56-128, called from float8_tensor.py:433-447),
// which torchao runs on SM 8.9 / XPU only (float8/inference.py:306-310).  The arithmetic (quant_math.h: fp8_block_acc, fp8_block_out):
//   casts: scale = f32(bf16(amax_block / 448)), the division in the input dtype;  q = e4m3_sat(f32(x) / scale)   (fp8_row_scale, fp8_quant8)
//          a block of zeros gives scale 0 and NaN codes, like the reference.  w bf16 [N][K], N and K multiples of 128 -> scale [N/128][K/128];
//          x bf16 [M][K] -> scale [M][K/128]; no row-wide amax pass.
//   GEMM, per output element, in fp32:
//          acc = 0
//          for kb ascending within a K part:
//            p    = sum over the block's 128 k of a[m][k] b[n][k]         (ONE v_mfma_scale_f32_16x16x128_f8f6f4 onto a zero accumulator)
//            acc += (p * a_s[m][kb]) * b_s[n / 128][kb]                    (two products and a sum, each rounded)
//          t = bf16(acc);  y = bias ? bf16(f32(t) + f32(bias[n])) : t      (rounded to bf16 BEFORE the bias, float8_tensor.py:445-447)
//   K parts (the waves of the stream form's workgroup) are cut at multiples of 128 and added in part order: a launch is reproducible.
//   Any N >= 1: b_s has ceil(N / 128) rows; ragged N and M are masked (kernels.py's offs_n // BLOCK_SIZE_K).  K a positive multiple of 128.
//
// The grouped GEMM for MoE experts (ao_fp8_block_grouped_mm; the reference has it as a training prototype only,
// prototype/moe_training/blockwise_fp8/grouped_mm.py over DeepGEMM or the bf16 emulation of blockwise_fp8_training/grouped_kernels.py:78-93)
// applies the same chain, without a bias, per token group [offs[e-1], offs[e]) against expert e: fp8_block_grouped_stream_kernel (grid
// (ceil(N / 16), E), the group's rows 16 MT at a time) and the GROUPED instantiation of fp8_block_tile_kernel, routed on the mean group
// size (grouped_route).
//
// Two forms, one route (block_route: this family's shape check, seam and forced form over the plans of two_form_route.h)
// read by the launches and by ao_fp8_block_linear_route / ao_fp8_block_linear_kernel_name:
//   fp8_block_stream_kernel: the weight is streamed once; a workgroup owns 16 columns and 16 / 32 / 64 rows and splits K over its waves
//     in 128-k steps; a step is the MFMA onto zero, four products with the a_s of the lane's rows 4 kq + {0..3} and one wave-uniform b_s
//     (a 16-column tile never crosses a 128-row scale boundary).  The partial tiles are parked in LDS (park_tile) and added in wave
//     order.  CAST: the 1 x 128 cast runs inside on the lanes that feed the A operand, with the stand-alone cast's functions, so the
//     result is bit-identical to cast + this kernel.
//   fp8_block_tile_kernel: 128 x 128 output tiles, four waves of 64 x 64, both operands staged in LDS by buffer_load ... lds, two stages;
//     b_s is one value per tile per K block.  A first cut: correct for every M and ragged N; not tuned.
// The seam: the stream form up to kStreamMaxRows = 192 rows (64 rows a grid row), the tiled form beyond -- where the two forms forced over
// M = 16 .. 256 on the Llama-3-8B five shapes cost least in sum (profiles/fp8_block_linear.jsonl).
#include "common.h"
#include "quant_math.h"
#include "stream_blocks.h"
#include "two_form_route.h"

namespace ao {
namespace {

// ---- the route ------------------------------------------------------------------------------------------------------------------
constexpr int kStreamMaxRows = AO_FP8_BLOCK_STREAM_MAX_ROWS;

thread_local int g_form = 0;  // ao_fp8_block_linear_set_form: 0 the product route, 1 stream, 2 tile

bool block_shape_ok(int64_t M, int64_t N, int64_t K) {
  if (M < 0 || N < 1 || K < 128 || K % 128 != 0) return false;
  if (M >= (1ll << 31) || N >= (1ll << 31) || K >= (1ll << 31)) return false;
  // each operand below 2 GiB: the buffer ranges of the tile form and the k offsets of both forms are 32-bit
  return M * K < (1ll << 31) && N * K < (1ll << 31) && M * N < (1ll << 40);
}

// kernel 1: fp8_block_stream_kernel, 2: fp8_block_tile_kernel (128 x 128 tiles)
TwoFormRoute block_route(int64_t M, int64_t N, int64_t K) {
  if (!block_shape_ok(M, N, K)) return TwoFormRoute{};
  return two_form_route(g_form != 0 ? g_form : (M <= kStreamMaxRows ? 1 : 2), M, N, K, 128);
}

struct BlockArgs {
  const uint8_t* a;       // codes [M][K] (stream form without CAST, tile form)
  const float* a_scale;   // [M][K/128]
  const uint16_t* x;      // bf16 [M][K] (CAST)
  const uint8_t* b;       // codes [N][K]
  const float* b_scale;   // [ceil(N/128)][K/128]
  const uint16_t* bias;   // bf16 [N] or null
  uint16_t* out;          // bf16 [M][N]
  int M, N, K;
};

__device__ __forceinline__ u32x4 ld16(const uint8_t* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ u32x4 ld16(const uint16_t* p) { return *reinterpret_cast<const u32x4*>(p); }

// ---- the casts ------------------------------------------------------------------------------------------------------------------
// amax of the 32 bf16 a lane holds of one 128-block (NaN blocks are outside the contract, as in the rowwise cast: their amax is inf)
__device__ __forceinline__ float amax32(const u32x4& a0, const u32x4& a1, const u32x4& a2, const u32x4& a3) {
  bool has_nan = false;
  const float m = fmaxf(fmaxf(amax8(a0, has_nan), amax8(a1, has_nan)), fmaxf(amax8(a2, has_nan), amax8(a3, has_nan)));
  return has_nan ? INFINITY : m;
}

// 1 x 128: sixteen adjacent lanes own one block, 8 bf16 each
__global__ __launch_bounds__(256) void fp8_quant_block_1x128_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q,
                                                                    float* __restrict__ scale, int64_t blocks) {
  const int64_t blk = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (blk >= blocks) return;  // whole 16-lane groups exit together
  const int part = threadIdx.x & 15;
  const u32x4 v = reinterpret_cast<const u32x4*>(x + blk * 128)[part];
  bool has_nan = false;
  float m = amax8(v, has_nan);
  if (has_nan) m = INFINITY;
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
  const float s = fp8_row_scale(m);
  reinterpret_cast<u32x2*>(q + blk * 128)[part] = fp8_quant8(v, s);
  if (part == 0) scale[blk] = s;
}

// 128 x 128: a workgroup owns one block; thread t holds 8 bf16 (piece t & 15) of rows (t >> 4) + 16 i
__global__ __launch_bounds__(256) void fp8_quant_block_128x128_kernel(const uint16_t* __restrict__ w, uint8_t* __restrict__ q,
                                                                      float* __restrict__ scale, int K) {
  __shared__ float wmax[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t base = ((size_t)blockIdx.y * 128 + (tid >> 4)) * K + (size_t)blockIdx.x * 128 + (tid & 15) * 8;
  u32x4 v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(w + base + (size_t)16 * i * K));
  bool has_nan = false;
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) m = fmaxf(m, amax8(v[i], has_nan));
  if (has_nan) m = INFINITY;
  m = wave_max(m);
  if (lane == 0) wmax[wave] = m;
  __syncthreads();
  const float s = fp8_row_scale(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
  if (tid == 0) scale[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
#pragma unroll
  for (int i = 0; i < 8; ++i) *reinterpret_cast<u32x2*>(q + base + (size_t)16 * i * K) = fp8_quant8(v[i], s);
}

// ---- streaming form -------------------------------------------------------------------------------------------------------------
// One lane's A operand of k block `step` for row `row` (rows past `rows` read as zero).
__device__ __forceinline__ void load_block_codes(const uint8_t* codes, int row, int rows, int step, int kq, int K, u32x4& v0, u32x4& v1) {
  v0 = u32x4{0u, 0u, 0u, 0u};
  v1 = v0;
  if (row < rows) {
    const uint8_t* p = codes + (size_t)row * K + step * 128 + 16 * kq;
    v0 = ld16(p);
    v1 = ld16(p + 64);
  }
}
// The same operand cast from the bf16 activation: the four lanes l & 15 of a row hold the block (k = 16 kq .. +15 and 64 + 16 kq .. +15),
// its amax meets across them; s is the block's scale on every one of the four.  Every lane runs the shuffles.
__device__ __forceinline__ void cast_block_operand(const uint16_t* x, int row, int rows, int step, int kq, int K, u32x4& v0, u32x4& v1,
                                                   float& s) {
  const u32x4 z = {0u, 0u, 0u, 0u};
  const bool rv = row < rows;
  const uint16_t* p = x + (size_t)(rv ? row : 0) * K + step * 128 + 16 * kq;
  const u32x4 a0 = rv ? ld16(p) : z, a1 = rv ? ld16(p + 8) : z, a2 = rv ? ld16(p + 64) : z, a3 = rv ? ld16(p + 72) : z;
  float m = amax32(a0, a1, a2, a3);
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  s = fp8_row_scale(m);
  const u32x2 c0 = fp8_quant8(a0, s), c1 = fp8_quant8(a1, s), c2 = fp8_quant8(a2, s), c3 = fp8_quant8(a3, s);
  v0 = rv ? u32x4{c0.x, c0.y, c1.x, c1.y} : z;  // (a row past M is a block of zeros: its codes would be NaN)
  v1 = rv ? u32x4{c2.x, c2.y, c3.x, c3.y} : z;
  if (!rv) s = 0.f;
}

template <bool CAST, int MT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void fp8_block_stream_kernel(BlockArgs p) {
  __shared__ float red[WAVES][MT][256];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kq = lane >> 4, nl = lane & 15;
  const int n = blockIdx.x * 16 + nl;
  const int m0 = blockIdx.y * 16 * MT;
  const int kblocks = p.K >> 7;
  const int ks0 = (kblocks * wave) / WAVES, ks1 = (kblocks * (wave + 1)) / WAVES;
  const bool nv = n < p.N;
  const uint8_t* brow = p.b + (size_t)(nv ? n : 0) * p.K + 16 * kq;
  // the tile's 16 columns lie in one 128-row block of the weight: blockIdx.x * 16 / 128
  const float* bs_row = p.b_scale + (size_t)(blockIdx.x >> 3) * kblocks;
  const u32x4 z = {0u, 0u, 0u, 0u};
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int step = ks0; step < ks1; ++step) {
    const u32x4 b0 = nv ? ld16(brow + step * 128) : z, b1 = nv ? ld16(brow + step * 128 + 64) : z;
    const float bs = bs_row[step];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      u32x4 a0, a1;
      f32x4 as;
      if constexpr (CAST) {
        float s;
        cast_block_operand(p.x, m0 + mt * 16 + nl, p.M, step, kq, p.K, a0, a1, s);
        // lane 4 kq + r holds row 4 kq + r of the tile
        as = f32x4{__shfl(s, 4 * kq), __shfl(s, 4 * kq + 1), __shfl(s, 4 * kq + 2), __shfl(s, 4 * kq + 3)};
      } else {
        load_block_codes(p.a, m0 + mt * 16 + nl, p.M, step, kq, p.K, a0, a1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + mt * 16 + 4 * kq + r;
          as[r] = row < p.M ? p.a_scale[(size_t)row * kblocks + step] : 0.f;
        }
      }
      const f32x4 prod = mfma8_k128<false>(a0, a1, b0, b1, f32x4{0.f, 0.f, 0.f, 0.f});
      acc[mt] = fp8_block_acc(acc[mt], prod, as, bs);
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) park_tile(&red[wave][mt][0], kq, nl, acc[mt]);
  __syncthreads();
  // the partial tiles are added in wave order
  const bool has_bias = p.bias != nullptr;
  for (int idx = threadIdx.x; idx < MT * 256; idx += 64 * WAVES) {
    const int mt = idx >> 8, rc = idx & 255;
    const int row = m0 + mt * 16 + (rc >> 4), col = blockIdx.x * 16 + (rc & 15);
    if (row < p.M && col < p.N) {
      float sum = red[0][mt][rc];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) sum += red[w][mt][rc];
      p.out[(size_t)row * p.N + col] = f32_to_bf16_bits(fp8_block_out(sum, has_bias, has_bias ? bf16_lo_to_f32(p.bias[col]) : 0.f));
    }
  }
}

// ---- grouped (MoE experts) ------------------------------------------------------------------------------------------------------
// Token group e = rows [offs[e-1], offs[e]) of a (offs[-1] = 0) against expert e's weight b[e] and scales b_scale[e]; the dense chain
// per element, no bias.  The kernels only read offs: a group's bounds are clamped to [0, M_total] (a bad offs cannot address outside a
// or out) and a non-increasing pair is an empty group.
struct GroupedArgs {
  const uint8_t* a;       // codes [M_total][K]
  const float* a_scale;   // [M_total][K/128]
  const uint8_t* b;       // codes [E][N][K]
  const float* b_scale;   // [E][ceil(N/128)][K/128]
  const int32_t* offs;    // [E] cumulative group ends
  uint16_t* out;          // bf16 [M_total][N]
  int M_total, N, K, E;
};

__device__ __forceinline__ int clamp_row(int r, int M_total) { return r < 0 ? 0 : (r > M_total ? M_total : r); }
__device__ __forceinline__ void group_bounds(const GroupedArgs& p, int e, int& row_begin, int& row_end) {
  row_begin = clamp_row(e > 0 ? p.offs[e - 1] : 0, p.M_total);
  row_end = clamp_row(p.offs[e], p.M_total);
}

// ---- LDS-tiled form -------------------------------------------------------------------------------------------------------------
// Stage layout: A then B, 128 rows of 128 bytes each, the eight 16-byte pieces of a row swizzled by row so that the 16 lanes of a
// fragment read hit different banks: piece c of row r sits at slot r * 8 + (c ^ (r % 8)).
constexpr int kOpBytes = 128 * 128;
constexpr int kStageBytes = 2 * kOpBytes;

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, char* lds, uint32_t voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds, 16, voff, 0, 0, 0);
}

__device__ __forceinline__ void tile_issue(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb, char* stage, int m0, int n0, int step, int M, int N,
                                           int K, int wave, int lane) {
  constexpr int kInstr = kOpBytes / 1024;  // 1 KiB per wave instruction
#pragma unroll
  for (int i = wave; i < 2 * kInstr; i += 4) {
    const bool isb = i >= kInstr;
    const int j = isb ? i - kInstr : i;
    const int slot = j * 64 + lane;
    const int r = slot >> 3, c = (slot & 7) ^ (r & 7);
    const int grow = (isb ? n0 : m0) + r;
    // rows past the matrix get an offset past any buffer's range (operands are below 2 GiB) and read as zero
    const uint32_t voff = grow < (isb ? N : M) ? (uint32_t)grow * (uint32_t)K + (uint32_t)(step * 128 + c * 16) : 0xFFFFFFF0u;
    dma16(isb ? rb : ra, stage + (isb ? kOpBytes : 0) + j * 1024, voff);
  }
}

__device__ __forceinline__ void tile_frag(const char* op, int r, int kq, u32x4& v0, u32x4& v1) {
  v0 = *reinterpret_cast<const u32x4*>(op + (r * 8 + (kq ^ (r & 7))) * 16);
  v1 = *reinterpret_cast<const u32x4*>(op + (r * 8 + ((kq + 4) ^ (r & 7))) * 16);
}

// 128 x 128 output tiles by workgroups of four waves: ONE body, two instantiations.
//   GROUPED false, "fp8_block_tile_kernel": the dense linear; q is the problem, the tile row is blockIdx.y.
//   GROUPED true, "fp8_block_grouped_tile_kernel": grid y is the host's upper bound ceil(M_total / 128) + E on the 128-row tiles of all
//     groups (a group adds at most one partial tile); a workgroup finds its (group, tile) by walking offs and leaves when it has none;
//     p is then the group's row window [row_begin, row_end) against its expert, expressed by offset base pointers (so the buffer
//     ranges end at the window).
// A template and not a device function called by two kernels: as an always-inline function the same body compiled to 256 + 36
// registers in the dense kernel (one wave a SIMD) where this form keeps the 224 + 4 (two waves a SIMD) it had before the grouped GEMM.
template <bool GROUPED>
__global__ __launch_bounds__(256) void fp8_block_tile_kernel(std::conditional_t<GROUPED, GroupedArgs, BlockArgs> q) {
  unsigned tile_y = blockIdx.y;
  BlockArgs p;
  if constexpr (GROUPED) {
    int t = blockIdx.y, e = 0, row_begin = 0, row_end = 0;
    for (; e < q.E; ++e) {
      group_bounds(q, e, row_begin, row_end);
      const int tiles = row_end > row_begin ? (row_end - row_begin + 127) >> 7 : 0;
      if (t < tiles) break;
      t -= tiles;
    }
    if (e == q.E) return;
    const int kb = q.K >> 7;
    p = BlockArgs{q.a + (size_t)row_begin * q.K, q.a_scale + (size_t)row_begin * kb, nullptr, q.b + (size_t)e * q.N * q.K,
                  q.b_scale + (size_t)e * ((q.N + 127) >> 7) * kb, nullptr, q.out + (size_t)row_begin * q.N, row_end - row_begin, q.N, q.K};
    tile_y = t;
  } else {
    p = q;
  }
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4;
  const int m0 = tile_y * 128, n0 = blockIdx.x * 128;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int kblocks = p.K >> 7;
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, 0, p.M * p.K, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)p.b, 0, p.N * p.K, 0x00020000);
  const float* bs_row = p.b_scale + (size_t)blockIdx.x * kblocks;  // one scale per tile per K block
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the a_s of the lane's output rows m0 + wm + 16 i + 4 kq + r, one K block ahead
  auto scales_at = [&](f32x4 (&as)[4], int step) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + 16 * i + 4 * kq + r;
        as[i][r] = row < p.M ? p.a_scale[(size_t)row * kblocks + step] : 0.f;
      }
  };
  f32x4 as[4];
  scales_at(as, 0);
  tile_issue(ra, rb, smem, m0, n0, 0, p.M, p.N, p.K, wave, lane);
  for (int step = 0; step < kblocks; ++step) {
    char* cur = smem + (step & 1) * kStageBytes;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage `step` has landed for every wave; every wave is done with the other stage
    f32x4 nas[4];
    if (step + 1 < kblocks) {
      tile_issue(ra, rb, smem + ((step + 1) & 1) * kStageBytes, m0, n0, step + 1, p.M, p.N, p.K, wave, lane);
      scales_at(nas, step + 1);
    }
    const float bs = bs_row[step];
    u32x4 bf0[4], bf1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) tile_frag(cur + kOpBytes, wn + 16 * j + (lane & 15), kq, bf0[j], bf1[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 a0, a1;
      tile_frag(cur, wm + 16 * i + (lane & 15), kq, a0, a1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 prod = mfma8_k128<false>(a0, a1, bf0[j], bf1[j], f32x4{0.f, 0.f, 0.f, 0.f});
        acc[i][j] = fp8_block_acc(acc[i][j], prod, as[i], bs);
      }
    }
    if (step + 1 < kblocks) {
#pragma unroll
      for (int i = 0; i < 4; ++i) as[i] = nas[i];
    }
  }
  const bool has_bias = p.bias != nullptr;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn + 16 * j + (lane & 15);
    if (n >= p.N) continue;
    const float bias = has_bias ? bf16_lo_to_f32(p.bias[n]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + 16 * i + 4 * kq + r;
        if (row < p.M) p.out[(size_t)row * p.N + n] = f32_to_bf16_bits(fp8_block_out(acc[i][j][r], has_bias, bias));
      }
  }
}

// ---- grouped streaming form -----------------------------------------------------------------------------------------------------
// Grid (ceil(N / 16), E): a workgroup owns 16 columns of one expert and walks its group's rows 16 MT at a time; per pass the step of
// fp8_block_stream_kernel (the weight block comes from L2 from the second pass on), the meeting in wave order, and a barrier before
// the next pass reuses the meeting buffer.
template <int MT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void fp8_block_grouped_stream_kernel(GroupedArgs p) {
  __shared__ float red[WAVES][MT][256];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kq = lane >> 4, nl = lane & 15;
  const int e = blockIdx.y;
  int row_begin, row_end;
  group_bounds(p, e, row_begin, row_end);
  if (row_end <= row_begin) return;  // an empty group: the whole workgroup leaves
  const int n = blockIdx.x * 16 + nl;
  const int kblocks = p.K >> 7;
  const int ks0 = (kblocks * wave) / WAVES, ks1 = (kblocks * (wave + 1)) / WAVES;
  const bool nv = n < p.N;
  // the expert's base in 64 bits: the whole b may pass 2 GiB
  const uint8_t* brow = p.b + (size_t)e * p.N * p.K + (size_t)(nv ? n : 0) * p.K + 16 * kq;
  const float* bs_row = p.b_scale + ((size_t)e * ((p.N + 127) >> 7) + (blockIdx.x >> 3)) * kblocks;
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (int m0 = row_begin; m0 < row_end; m0 += 16 * MT) {
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int step = ks0; step < ks1; ++step) {
      const u32x4 b0 = nv ? ld16(brow + step * 128) : z, b1 = nv ? ld16(brow + step * 128 + 64) : z;
      const float bs = bs_row[step];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        u32x4 a0, a1;
        f32x4 as;
        load_block_codes(p.a, m0 + mt * 16 + nl, row_end, step, kq, p.K, a0, a1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + mt * 16 + 4 * kq + r;
          as[r] = row < row_end ? p.a_scale[(size_t)row * kblocks + step] : 0.f;
        }
        const f32x4 prod = mfma8_k128<false>(a0, a1, b0, b1, f32x4{0.f, 0.f, 0.f, 0.f});
        acc[mt] = fp8_block_acc(acc[mt], prod, as, bs);
      }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) park_tile(&red[wave][mt][0], kq, nl, acc[mt]);
    __syncthreads();
    // the partial tiles are added in wave order
    for (int idx = threadIdx.x; idx < MT * 256; idx += 64 * WAVES) {
      const int mt = idx >> 8, rc = idx & 255;
      const int row = m0 + mt * 16 + (rc >> 4), col = blockIdx.x * 16 + (rc & 15);
      if (row < row_end && col < p.N) {
        float sum = red[0][mt][rc];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) sum += red[w][mt][rc];
        p.out[(size_t)row * p.N + col] = f32_to_bf16_bits(fp8_block_out(sum));
      }
    }
    __syncthreads();  // the next pass parks into the same buffer
  }
}

// ---- launches -------------------------------------------------------------------------------------------------------------------
// (4 m-tiles x 16 waves: the meeting buffer would pass the static LDS; the stream-form plan caps 4 m-tiles at 8 waves)
template <bool CAST>
int launch_stream(const TwoFormRoute& r, const BlockArgs& a, hipStream_t st) {
  return launch_stream_form<false>("fp8_block_stream_kernel", "fp8_block_stream_kernel launch", r, a, st, [](auto mt, auto waves) {
    return fp8_block_stream_kernel<CAST, decltype(mt)::value, decltype(waves)::value>;
  });
}

int launch_tile(const TwoFormRoute& r, const BlockArgs& a, hipStream_t st) {
  return launch_tile_form(fp8_block_tile_kernel<false>, "fp8_block_tile_kernel launch", r, a, st, 2 * kStageBytes,
                          "hipFuncSetAttribute(fp8_block_tile_kernel)");
}

int check_linear(const char* fn, int64_t M, int64_t N, int64_t K) {
  AO_REQUIRE(block_shape_ok(M, N, K), "%s: bad shape M=%lld N=%lld K=%lld (M >= 0, N >= 1, K a positive multiple of 128, operands < 2 GiB)", fn,
             (long long)M, (long long)N, (long long)K);
  return AO_OK;
}

// ---- the grouped route ------------------------------------------------------------------------------------------------------------
// (on the mean group size: grouped_two_form_route)
constexpr int kGroupedStreamMaxRows = AO_FP8_BLOCK_GROUPED_STREAM_MAX_ROWS;

thread_local int g_grouped_form = 0;  // ao_fp8_block_grouped_mm_set_form: 0 the product route, 1 stream, 2 tile

bool grouped_shape_ok(int64_t M_total, int64_t N, int64_t K, int64_t E) {
  if (E < 1 || E > 65535) return false;
  return block_shape_ok(M_total, N, K);  // M_total K and the per-expert N K below 2 GiB; the expert base is 64-bit
}

// kernel 1: fp8_block_grouped_stream_kernel, grid (ceil(N / 16), E), m-tiles and waves of the stream plan at the mean group size;
// 2: fp8_block_grouped_tile_kernel = fp8_block_tile_kernel<true>, grid (ceil(N / 128), ceil(M_total / 128) + E)
TwoFormRoute grouped_route(int64_t M_total, int64_t N, int64_t K, int64_t E) {
  if (!grouped_shape_ok(M_total, N, K, E)) return TwoFormRoute{};
  return grouped_two_form_route(g_grouped_form, kGroupedStreamMaxRows, M_total, N, K, E, 128);
}

int launch_grouped_stream(const TwoFormRoute& r, const GroupedArgs& a, hipStream_t st) {
  return launch_stream_form<false>("fp8_block_grouped_stream_kernel", "fp8_block_grouped_stream_kernel launch", r, a, st,
                                   [](auto mt, auto waves) { return fp8_block_grouped_stream_kernel<decltype(mt)::value, decltype(waves)::value>; });
}

int launch_grouped_tile(const TwoFormRoute& r, const GroupedArgs& a, hipStream_t st) {
  return launch_tile_form(fp8_block_tile_kernel<true>, "fp8_block_grouped_tile_kernel (fp8_block_tile_kernel<GROUPED>) launch", r, a, st,
                          2 * kStageBytes, "hipFuncSetAttribute(fp8_block_tile_kernel<GROUPED>)");
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_fp8_quantize_block_1x128(const uint16_t* x, uint8_t* q, float* scale, int64_t M, int64_t K, void* stream) {
  AO_REQUIRE(M >= 0 && K >= 128 && K % 128 == 0, "%s: bad shape M=%lld K=%lld (K must be a positive multiple of 128)", __func__, (long long)M,
             (long long)K);
  AO_REQUIRE(M < (1ll << 31) && K < (1ll << 31) && M * K < (1ll << 40), "%s: M=%lld K=%lld too large for one launch", __func__, (long long)M,
             (long long)K);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(scale);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(q, 16) && aligned_to(scale, 4), "%s: x and q must be 16-byte, scale 4-byte aligned", __func__);
  const int64_t blocks = M * (K / 128);
  const int64_t grid = (blocks + 15) / 16;
  AO_REQUIRE(grid < (1ll << 31), "%s: tensor too large for one launch", __func__);
  ao::launch(fp8_quant_block_1x128_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), x, q, scale, blocks);
  AO_LAUNCH_CHECK("fp8_quant_block_1x128_kernel launch");
  return AO_OK;
}

extern "C" int ao_fp8_quantize_block_128x128(const uint16_t* w, uint8_t* q, float* scale, int64_t N, int64_t K, void* stream) {
  AO_REQUIRE(N >= 0 && N % 128 == 0 && K >= 128 && K % 128 == 0,
             "%s: bad shape N=%lld K=%lld (N must be a multiple of 128, K a positive multiple of 128)", __func__, (long long)N, (long long)K);
  AO_REQUIRE(K < (1ll << 31) && N / 128 <= 65535, "%s: N=%lld K=%lld too large for one launch", __func__, (long long)N, (long long)K);
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(scale);
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(q, 16) && aligned_to(scale, 4), "%s: w and q must be 16-byte, scale 4-byte aligned", __func__);
  ao::launch(fp8_quant_block_128x128_kernel, dim3((unsigned)(K / 128), (unsigned)(N / 128)), dim3(256), 0, static_cast<hipStream_t>(stream), w,
             q, scale, (int)K);
  AO_LAUNCH_CHECK("fp8_quant_block_128x128_kernel launch");
  return AO_OK;
}

extern "C" int ao_fp8_block_linear_route(int64_t M, int64_t N, int64_t K, int32_t* out, int cap) {
  return route_export(__func__, block_route(M, N, K), out, cap);
}

extern "C" const char* ao_fp8_block_linear_kernel_name(int64_t M, int64_t N, int64_t K) {
  return route_kernel_name(block_route(M, N, K), "fp8_block_stream_kernel", "fp8_block_tile_kernel");
}

extern "C" int ao_fp8_block_linear_set_form(int form) { return set_forced_form(__func__, form, g_form); }

extern "C" int ao_fp8_block_linear(const uint8_t* a, const float* a_scale, const uint8_t* b, const float* b_scale, const uint16_t* bias,
                                   uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream) {
  if (int rc = check_linear(__func__, M, N, K)) return rc;
  AO_REQUIRE_PTR(b);
  AO_REQUIRE_PTR(b_scale);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(a);
  AO_REQUIRE_PTR(a_scale);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(a, 16) && aligned_to(b, 16), "%s: the codes must be 16-byte aligned", __func__);
  AO_REQUIRE(aligned_to(a_scale, 4) && aligned_to(b_scale, 4) && aligned_to(bias, 2) && aligned_to(out, 2),
             "%s: the scales must be 4-byte, bias and out 2-byte aligned", __func__);
  const TwoFormRoute r = block_route(M, N, K);
  AO_REQUIRE(r.kernel != 0, "%s: no route for M=%lld N=%lld K=%lld", __func__, (long long)M, (long long)N, (long long)K);
  const BlockArgs args{a, a_scale, nullptr, b, b_scale, bias, out, (int)M, (int)N, (int)K};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return r.kernel == 1 ? launch_stream<false>(r, args, st) : launch_tile(r, args, st);
}

extern "C" int ao_fp8_block_dynamic_linear_fits(int64_t M, int64_t N, int64_t K) { return block_route(M, N, K).kernel == 1 ? 1 : 0; }

extern "C" int ao_fp8_block_dynamic_linear(const uint16_t* x, const uint8_t* b, const float* b_scale, const uint16_t* bias, uint16_t* out,
                                           int64_t M, int64_t N, int64_t K, void* stream) {
  if (int rc = check_linear(__func__, M, N, K)) return rc;
  AO_REQUIRE_PTR(b);
  AO_REQUIRE_PTR(b_scale);
  const TwoFormRoute r = block_route(M, N, K);
  AO_REQUIRE(r.kernel == 1, "%s: M=%lld N=%lld K=%lld takes the tiled form: cast (ao_fp8_quantize_block_1x128) and call ao_fp8_block_linear",
             __func__, (long long)M, (long long)N, (long long)K);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(b, 16), "%s: x and the codes must be 16-byte aligned", __func__);
  AO_REQUIRE(aligned_to(b_scale, 4) && aligned_to(bias, 2) && aligned_to(out, 2), "%s: b_scale must be 4-byte, bias and out 2-byte aligned",
             __func__);
  const BlockArgs args{nullptr, nullptr, x, b, b_scale, bias, out, (int)M, (int)N, (int)K};
  return launch_stream<true>(r, args, static_cast<hipStream_t>(stream));
}

extern "C" int ao_fp8_block_grouped_mm_route(int64_t M_total, int64_t N, int64_t K, int64_t E, int32_t* out, int cap) {
  return route_export(__func__, grouped_route(M_total, N, K, E), out, cap);
}

extern "C" const char* ao_fp8_block_grouped_mm_kernel_name(int64_t M_total, int64_t N, int64_t K, int64_t E) {
  return route_kernel_name(grouped_route(M_total, N, K, E), "fp8_block_grouped_stream_kernel", "fp8_block_grouped_tile_kernel");
}

extern "C" int ao_fp8_block_grouped_mm_set_form(int form) { return set_forced_form(__func__, form, g_grouped_form); }

extern "C" int ao_fp8_block_grouped_mm(const uint8_t* a, const float* a_scale, const uint8_t* b, const float* b_scale, const int32_t* offs,
                                       uint16_t* out, int64_t M_total, int64_t N, int64_t K, int64_t E, void* stream) {
  AO_REQUIRE(grouped_shape_ok(M_total, N, K, E),
             "%s: bad shape M_total=%lld N=%lld K=%lld E=%lld (M_total >= 0, N >= 1, K a positive multiple of 128, 1 <= E <= 65535, "
             "M_total K and the per-expert N K < 2 GiB)",
             __func__, (long long)M_total, (long long)N, (long long)K, (long long)E);
  AO_REQUIRE_PTR(b);
  AO_REQUIRE_PTR(b_scale);
  AO_REQUIRE_PTR(offs);
  if (M_total == 0) return AO_OK;
  AO_REQUIRE_PTR(a);
  AO_REQUIRE_PTR(a_scale);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(a, 16) && aligned_to(b, 16), "%s: the codes must be 16-byte aligned", __func__);
  AO_REQUIRE(aligned_to(a_scale, 4) && aligned_to(b_scale, 4) && aligned_to(offs, 4) && aligned_to(out, 2),
             "%s: the scales and offs must be 4-byte, out 2-byte aligned", __func__);
  const TwoFormRoute r = grouped_route(M_total, N, K, E);
  AO_REQUIRE(r.kernel != 0, "%s: no route for M_total=%lld N=%lld K=%lld E=%lld (more than 65535 grid rows)", __func__, (long long)M_total,
             (long long)N, (long long)K, (long long)E);
  const GroupedArgs args{a, a_scale, b, b_scale, offs, out, (int)M_total, (int)N, (int)K, (int)E};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return r.kernel == 1 ? launch_grouped_stream(r, args, st) : launch_grouped_tile(r, args, st);
}
