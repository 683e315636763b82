// BitNet b1.58 (torchao/prototype/quantized_training/bitnet.py) on gfx950: ternary weights packed four to a byte, int8 activations, the
// product on v_mfma_i32_16x16x64_i8.  The arithmetic, every step ONE fp32 operation rounded once, the divisions IEEE:
//   absmean   scale = f32(sum |w| / numel), the sum and the quotient in float64: each workgroup leaves one float64 partial, a second launch
//             adds the partials in index order -- no floating-point atomics, the same bits on every run
//   weight    q = clip(rint(f32(w) / max(scale, 1e-5)), -1, 1);  byte j of a row = q[4j] << 6 | (q[4j+1] & 3) << 4 | (q[4j+2] & 3) << 2 |
//             (q[4j+3] & 3): field s of a byte sits at bits 7 - 2s .. 6 - 2s, the reference's _pack_i2_in_i8
//   act       s = bf16(amax_row / 127);  inv = 1 / max(f32(s), 1e-5);  q = clip(rint(f32(x) * inv), -128, 127)   (quantize_int8_rowwise, eps 1e-5)
//   mm        y = bf16((f32(acc) * f32(row_scale[m])) * f32(tensor_scale));  with a bias y = bf16(f32(y) + f32(bias[n])), a second rounding
//             acc = sum_k a[m][k] q[n][k] in int32: exact, so any k order and any K split give the same bits
// Both mm forms unpack in registers from those bytes: a 2-bit field, masked to 0 / 1 / 3 in a byte, is a v_perm_b32 selector into the table
// bytes (0, 1, -2, -1), so `(dword >> (6 - 2s)) & 0x03030303` + one v_perm_b32 gives field s of four packed bytes as four int8.
//   streaming (M <= 16)  a lane's dwordx4 of packed bytes holds 64 weights of one output row; field s of dword d is k = 16d + 4j + s, a
//             stride-4 set.  The k order inside an MFMA step is free (the sum is exact), so the activation rows are staged through LDS ONCE a
//             workgroup in that permuted order (a 4 x 4 byte transpose per 16 bytes) and the weights are never shuffled: 11 VALU operations a
//             packed dword.  A workgroup owns 16 output features, its four waves split K, the int32 partial tiles meet in LDS.
//   tiled (M > 16)       128 x 64 output tile, K steps of 64, three LDS stages.  A moves by global_load_lds in natural order (16-byte pieces
//             swizzled on the source side against bank conflicts); W moves by global_load_lds too and stays PACKED in LDS (16 bytes a row and
//             step); a lane reads one packed dword and unpacks it to natural k order (the four field words, then a 4 x 4 byte transpose:
//             19 operations a dword).  Operands swapped (W as the MFMA's A) so that a lane ends with four adjacent columns of one row.
#include "common.h"
#include "lds_dma.h"
#include "quant_math.h"

#include <algorithm>

namespace ao {
namespace {

constexpr int kAbsmeanMaxBlocks = AO_BITNET_ABSMEAN_WORKSPACE;  // the float64 workspace the caller brings

// ---- absmean ------------------------------------------------------------------------------------------------------------------------------
// sum over the kRowThreads threads of a workgroup in a fixed order (the wave butterfly gives every lane the same bits), in thread 0 at least
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(kRowThreads) void bitnet_absmean_partial_kernel(const uint16_t* w, int64_t numel, double* partial) {
  __shared__ double red[4];
  const int64_t nvec = numel >> 3;
  const u32x4* wv = reinterpret_cast<const u32x4*>(w);
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * kRowThreads) {
    float f[8];
    unpack_bf16x8(__builtin_nontemporal_load(wv + i), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += (double)fabsf(f[j]);
  }
  // the tail of a tensor whose size is no multiple of 8 (K % 4 == 0: four elements)
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (numel & 7)) acc += (double)fabsf(bf16_lo_to_f32(w[(nvec << 3) + threadIdx.x]));
  acc = block_sum_f64(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kRowThreads) void bitnet_absmean_finish_kernel(const double* partial, int nparts, int64_t numel, float* out,
                                                                            uint16_t* out_bf16) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kRowThreads) acc += partial[i];
  acc = block_sum_f64(acc, red);
  if (threadIdx.x == 0) {
    const float m = (float)(acc / (double)numel);
    *out = m;
    if (out_bf16 != nullptr) *out_bf16 = f32_to_bf16_bits(m);  // tensor_scale.to(weight.dtype), what the mm takes
  }
}

// ---- the weight cast (quant_math.h: bitnet_ternary) -----------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bitnet_pack4(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3) {
  return ((q0 & 3u) << 6) | ((q1 & 3u) << 4) | ((q2 & 3u) << 2) | (q3 & 3u);
}
__device__ __forceinline__ uint32_t bitnet_bytes4(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3) {
  return (q0 & 0xffu) | ((q1 & 0xffu) << 8) | ((q2 & 0xffu) << 16) | (q3 << 24);
}

// The tensor as a flat run of 8-element units (K % 4 == 0 keeps every group of four inside a row); the last unit may hold four.
__global__ __launch_bounds__(kRowThreads) void bitnet_quantize_weight_kernel(const uint16_t* w, const float* scale, uint8_t* packed, int8_t* q8,
                                                                             int64_t numel) {
  const float s = fmaxf(*scale, kBitnetEps);
  const int64_t units = (numel + 7) >> 3;
  for (int64_t u = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; u < units; u += (int64_t)gridDim.x * kRowThreads) {
    const bool full = (u << 3) + 8 <= numel;
    u32x4 v;
    if (full) {
      v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(w) + u);
    } else {
      const u32x2 h = *reinterpret_cast<const u32x2*>(w + (u << 3));
      v = u32x4{h.x, h.y, 0u, 0u};
    }
    float f[8];
    unpack_bf16x8(v, f);
    uint32_t q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = bitnet_ternary(f[j], s);
    const uint32_t b0 = bitnet_pack4(q[0], q[1], q[2], q[3]), b1 = bitnet_pack4(q[4], q[5], q[6], q[7]);
    if (full) *reinterpret_cast<uint16_t*>(packed + 2 * u) = (uint16_t)(b0 | (b1 << 8));
    else packed[2 * u] = (uint8_t)b0;
    if (q8 != nullptr) {
      const uint32_t lo = bitnet_bytes4(q[0], q[1], q[2], q[3]), hi = bitnet_bytes4(q[4], q[5], q[6], q[7]);
      if (full) *reinterpret_cast<u32x2*>(q8 + (u << 3)) = u32x2{lo, hi};
      else *reinterpret_cast<uint32_t*>(q8 + (u << 3)) = lo;
    }
  }
}

// ---- dequantize: packed bytes -> bf16 ternary values, no scale --------------------------------------------------------------------------------
// the bf16 bits of a field: 0 -> 0, 1 -> 1, 2 -> -2 (never written by the cast, but _unpack_i2_in_i8 reads it so), 3 -> -1
__device__ __forceinline__ uint32_t bitnet_field_bf16(uint32_t f) { return (uint32_t)(0xBF80C0003F800000ull >> (16u * f)) & 0xffffu; }
__device__ __forceinline__ u32x2 bitnet_byte_bf16x4(uint32_t b) {
  return u32x2{bitnet_field_bf16((b >> 6) & 3u) | (bitnet_field_bf16((b >> 4) & 3u) << 16),
               bitnet_field_bf16((b >> 2) & 3u) | (bitnet_field_bf16(b & 3u) << 16)};
}

__global__ __launch_bounds__(kRowThreads) void bitnet_dequantize_kernel(const uint8_t* packed, uint16_t* out, int64_t nbytes) {
  const int64_t ndw = nbytes >> 2;
  for (int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; i < ndw; i += (int64_t)gridDim.x * kRowThreads) {
    const uint32_t p = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(packed) + i);
    const u32x2 a = bitnet_byte_bf16x4(p & 0xffu), b = bitnet_byte_bf16x4((p >> 8) & 0xffu), c = bitnet_byte_bf16x4((p >> 16) & 0xffu),
                d = bitnet_byte_bf16x4(p >> 24);
    u32x4* o = reinterpret_cast<u32x4*>(out + (i << 4));
    o[0] = u32x4{a.x, a.y, b.x, b.y};
    o[1] = u32x4{c.x, c.y, d.x, d.y};
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (nbytes & 3)) {  // the bytes past the last whole dword
    const int64_t b = (ndw << 2) + threadIdx.x;
    *reinterpret_cast<u32x2*>(out + (b << 2)) = bitnet_byte_bf16x4(packed[b]);
  }
}

// ---- the activation cast: one workgroup a row, the second pass reads the row from cache ----------------------------------------------------------
__global__ __launch_bounds__(kRowThreads) void bitnet_quantize_act_kernel(const uint16_t* x, int8_t* q, uint16_t* scale, int K) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const u32x4* xr = reinterpret_cast<const u32x4*>(x + row * K);
  const int nvec = K >> 3;
  float m = 0.f;
  bool has_nan = false;  // (NaN rows are outside the contract)
  for (int i = threadIdx.x; i < nvec; i += kRowThreads) m = fmaxf(m, amax8(xr[i], has_nan));
  m = block_max(m, red);
  const float s = round_bf16(m / 127.0f);
  const float inv = 1.0f / fmaxf(s, kBitnetEps);
  for (int i = threadIdx.x; i < nvec; i += kRowThreads) *reinterpret_cast<u32x2*>(q + row * K + (i << 3)) = int8_quant8(xr[i], inv);
  if (threadIdx.x == 0) scale[row] = f32_to_bf16_bits(s);
}

// ---- the matmul ---------------------------------------------------------------------------------------------------------------------------------
struct BitnetMmArgs {
  const int8_t* a;               // [M][K]
  const uint8_t* w;              // [N][K / 4] packed
  const uint16_t* row_scale;     // [M] bf16
  const uint16_t* tensor_scale;  // one bf16
  const uint16_t* bias;          // [N] bf16 or null
  uint16_t* out;                 // [M][N] bf16
  int M, N, K;
};

constexpr uint32_t kTernaryTable = 0xFFFE0100u;  // v_perm_b32 source: selector 0 -> 0, 1 -> 1, 2 -> -2, 3 -> -1
// field s (0 .. 3) of the four bytes of a packed dword as four int8
template <int S>
__device__ __forceinline__ uint32_t bitnet_field_bytes(uint32_t p) {
  return __builtin_amdgcn_perm(0u, kTernaryTable, (S == 3 ? p : p >> (6 - 2 * S)) & 0x03030303u);
}
// y[j] = {x[0].byte j, x[1].byte j, x[2].byte j, x[3].byte j}
__device__ __forceinline__ u32x4 transpose_bytes4x4(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
  const uint32_t lo01 = __builtin_amdgcn_perm(x1, x0, 0x05010400u), hi01 = __builtin_amdgcn_perm(x1, x0, 0x07030602u);
  const uint32_t lo23 = __builtin_amdgcn_perm(x3, x2, 0x05010400u), hi23 = __builtin_amdgcn_perm(x3, x2, 0x07030602u);
  return u32x4{__builtin_amdgcn_perm(lo23, lo01, 0x05040100u), __builtin_amdgcn_perm(lo23, lo01, 0x07060302u),
               __builtin_amdgcn_perm(hi23, hi01, 0x05040100u), __builtin_amdgcn_perm(hi23, hi01, 0x07060302u)};
}
// (the output element from the exact sum: quant_math.h, bitnet_out)

// Streaming form.  grid (n-tiles of 16, m-tiles of 16), four waves.  LDS: red [4][256] int32, then the activation rows of one K chunk in
// the permuted order: k = 64 b + 4 t + s of a row sits at byte 64 b + 16 s + t, rows kStreamRowStride apart (16 bytes of padding: the 16 rows
// of a ds_read_b128 fall into different banks).
constexpr int kStreamChunk = 2048;                     // k per LDS fill
constexpr int kStreamRowStride = kStreamChunk + 16;
constexpr int kStreamRedBytes = 4 * 256 * 4;

__global__ __launch_bounds__(256) void bitnet_mm_stream_kernel(BitnetMmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* red = reinterpret_cast<int*>(smem);
  char* xs = smem + kStreamRedBytes;
  const int tid = threadIdx.x, lane = tid & 63, nl = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.y * 16, n0 = blockIdx.x * 16;
  const int rows = min(16, p.M - m0);
  const uint8_t* wrow = p.w + (size_t)min(n0 + nl, p.N - 1) * (size_t)(p.K >> 2);  // (columns past N: a valid row, never stored)

  i32x4 acc = {0, 0, 0, 0};
  for (int k0 = 0; k0 < p.K; k0 += kStreamChunk) {
    const int kspan = min(kStreamChunk, p.K - k0);  // a multiple of 64
    if (k0 != 0) __syncthreads();                   // the previous chunk has been read
    const int pieces = kspan >> 4;
    for (int u = tid; u < rows * pieces; u += 256) {
      const int r = u / pieces, pc = u - r * pieces;
      const u32x4 v = *reinterpret_cast<const u32x4*>(p.a + (size_t)(m0 + r) * p.K + k0 + (pc << 4));
      // dword i of the piece is t = 4 (pc & 3) + i, its byte s is field position s: word s of the transpose goes to byte 16 s + 4 (pc & 3)
      const u32x4 y = transpose_bytes4x4(v.x, v.y, v.z, v.w);
      char* dst = xs + r * kStreamRowStride + ((pc >> 2) << 6) + ((pc & 3) << 2);
      *reinterpret_cast<uint32_t*>(dst) = y.x;
      *reinterpret_cast<uint32_t*>(dst + 16) = y.y;
      *reinterpret_cast<uint32_t*>(dst + 32) = y.z;
      *reinterpret_cast<uint32_t*>(dst + 48) = y.w;
    }
    __syncthreads();
    const int steps = (kspan + 255) >> 8;  // 256 k a wave step: lane group kq takes the 64-k block 4 step + kq
    for (int st = wave; st < steps; st += 4) {
      const int b = st * 4 + kq;
      const bool live = (b << 6) < kspan;
      u32x4 wp = {0u, 0u, 0u, 0u};  // (field 0 reads as weight 0)
      if (live) wp = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow + ((k0 + (b << 6)) >> 2)));
      const char* xa = xs + nl * kStreamRowStride + (b << 6);
      const bool has_row = live && nl < rows;
      auto step = [&](auto s) {
        constexpr int S = decltype(s)::value;
        const i32x4 wop = {(int)bitnet_field_bytes<S>(wp.x), (int)bitnet_field_bytes<S>(wp.y), (int)bitnet_field_bytes<S>(wp.z),
                           (int)bitnet_field_bytes<S>(wp.w)};
        i32x4 aop = {0, 0, 0, 0};
        if (has_row) aop = *reinterpret_cast<const i32x4*>(xa + S * 16);
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(aop, wop, acc, 0, 0, 0);
      };
      step(std::integral_constant<int, 0>{});
      step(std::integral_constant<int, 1>{});
      step(std::integral_constant<int, 2>{});
      step(std::integral_constant<int, 3>{});
    }
  }
  // the waves' K shares meet: lane (column nl, group kq) holds rows 4 kq .. + 3
  int* r = red + wave * 256 + (kq * 4) * 16 + nl;
  r[0] = acc.x; r[16] = acc.y; r[32] = acc.z; r[48] = acc.w;
  __syncthreads();
  const int row = tid >> 4, n = n0 + (tid & 15);
  if (row < rows && n < p.N) {
    const int sum = (red[tid] + red[256 + tid]) + (red[512 + tid] + red[768 + tid]);
    const int m = m0 + row;
    p.out[(size_t)m * p.N + n] = bitnet_out(sum, bf16_lo_to_f32(p.row_scale[m]), bf16_lo_to_f32(*p.tensor_scale), p.bias != nullptr,
                                            p.bias != nullptr ? bf16_lo_to_f32(p.bias[n]) : 0.f);
  }
}

// Tiled form.  grid (n-tiles of 64, m-tiles of 128), four waves as 2 x 2, a wave owns 64 rows x 32 columns = 4 x 2 MFMA tiles.
// LDS stage: A [128 rows][64 bytes], the 16-byte piece c of row r at slot c ^ ((r >> 2) & 3); W [64 rows][16 packed bytes].
constexpr int kTileM = 128, kTileN = 64, kTileK = 64, kTileStages = 3;
constexpr int kTileABytes = kTileM * kTileK, kTileWBytes = kTileN * (kTileK / 4);
constexpr int kTileDmaPerStep = 3;  // DMA instructions a wave issues per step: two for A, one for W

__global__ __launch_bounds__(256) void bitnet_mm_tile_kernel(BitnetMmArgs p) {
  __shared__ __attribute__((aligned(16))) char As[kTileStages][kTileABytes];
  __shared__ __attribute__((aligned(16))) char Ws[kTileStages][kTileWBytes];
  const int tid = threadIdx.x, lane = tid & 63, ml = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * kTileM, n0 = blockIdx.x * kTileN;
  const int T = p.K / kTileK;

  // this lane's DMA sources; rows and columns past the edge read the last valid one (never stored)
  const int ar = 32 * wave + (lane >> 2);  // the row of the first A instruction, the second takes row + 16 (same swizzle: (r >> 2) & 3 = lane >> 4)
  const uint32_t apiece = (uint32_t)(((lane & 3) ^ (lane >> 4)) << 4);
  const uint32_t av0 = (uint32_t)min(ar, p.M - 1 - m0) * (uint32_t)p.K + apiece;
  const uint32_t av1 = (uint32_t)min(ar + 16, p.M - 1 - m0) * (uint32_t)p.K + apiece;
  const uint32_t wv = (uint32_t)min(16 * wave + (lane >> 2), p.N - 1 - n0) * (uint32_t)(p.K >> 2) + (uint32_t)((lane & 3) << 2);
  const char* abase = reinterpret_cast<const char*>(p.a) + (size_t)m0 * p.K;
  const char* wbase = reinterpret_cast<const char*>(p.w) + (size_t)n0 * (size_t)(p.K >> 2);
  auto issue = [&](int t) {
    const int buf = t % kTileStages;
    dma_b128_x2(abase + (size_t)t * kTileK, av0, av1, lds_offset(As[buf]) + wave * 2048);
    dma_b32_s(wbase + (size_t)t * (kTileK / 4), wv, lds_offset(Ws[buf]) + wave * 256);
  };

  i32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

  issue(0);
  if (T > 1) issue(1);
  for (int t = 0; t < T; ++t) {
    // step t has landed for this wave (the DMAs return in order); past the barrier for all of them, and stage (t + 2) % 3 = (t - 1) % 3 is read out
    if (t + 1 < T) wait_vmcnt<kTileDmaPerStep>();
    else wait_vmcnt<0>();
    lds_barrier();
    if (t + 2 < T) issue(t + 2);
    const char* A = As[t % kTileStages];
    const char* W = Ws[t % kTileStages];
    i32x4 wop[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t pk = *reinterpret_cast<const uint32_t*>(W + (wn * 32 + j * 16 + ml) * 16 + kq * 4);  // k = 16 kq + 4 byte + field
      wop[j] = __builtin_bit_cast(i32x4, transpose_bytes4x4(bitnet_field_bytes<0>(pk), bitnet_field_bytes<1>(pk), bitnet_field_bytes<2>(pk),
                                                           bitnet_field_bytes<3>(pk)));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = wm * 64 + i * 16 + ml;
      const i32x4 aop = *reinterpret_cast<const i32x4*>(A + r * kTileK + ((kq ^ ((ml >> 2) & 3)) << 4));
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wop[j], aop, acc[i][j], 0, 0, 0);
    }
  }

  // W was the MFMA's A: lane (row ml of the m-tile, group kq) holds columns 4 kq .. + 3 of the n-tile
  const float ts = bf16_lo_to_f32(*p.tensor_scale);
  const bool has_bias = p.bias != nullptr;
  const bool wide = (p.N & 3) == 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + ml;
    if (m >= p.M) continue;
    const float rs = bf16_lo_to_f32(p.row_scale[m]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 32 + j * 16 + kq * 4;
      uint16_t o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] = bitnet_out(acc[i][j][e], rs, ts, has_bias, (has_bias && n + e < p.N) ? bf16_lo_to_f32(p.bias[n + e]) : 0.f);
      uint16_t* dst = p.out + (size_t)m * p.N + n;
      if (wide && n + 3 < p.N) {
        *reinterpret_cast<u32x2*>(dst) = u32x2{(uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16)};
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < p.N) dst[e] = o[e];
      }
    }
  }
}

int bitnet_mm_check_shape(const char* fn, int64_t M, int64_t N, int64_t K) {
  AO_REQUIRE(M >= 0 && N >= 0 && K > 0, "%s: bad shape M=%lld N=%lld K=%lld", fn, (long long)M, (long long)N, (long long)K);
  AO_REQUIRE(K % 64 == 0, "%s: K=%lld must be a multiple of 64 (one v_mfma_i32_16x16x64_i8 step of packed 2-bit weights)", fn, (long long)K);
  AO_REQUIRE(M <= (1ll << 19) && N <= (1ll << 24) && K <= (1ll << 24), "%s: M=%lld N=%lld K=%lld too large (M <= 2^19, N and K <= 2^24)", fn,
             (long long)M, (long long)N, (long long)K);
  return AO_OK;
}

int grid_for(int64_t work_items) { return (int)std::max<int64_t>(1, std::min<int64_t>((work_items + kRowThreads - 1) / kRowThreads, 4096)); }

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_bitnet_absmean(const uint16_t* w, int64_t numel, double* workspace, float* out, uint16_t* out_bf16, void* stream) {
  AO_REQUIRE(numel > 0 && numel % 4 == 0, "%s: numel=%lld must be a positive multiple of 4", __func__, (long long)numel);
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(workspace);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(w, 16), "%s: w must be 16-byte aligned", __func__);
  const int blocks = std::min(grid_for(numel >> 3), kAbsmeanMaxBlocks);
  ao::launch(bitnet_absmean_partial_kernel, dim3(blocks), dim3(kRowThreads), 0, (hipStream_t)stream, w, numel, workspace);
  AO_LAUNCH_CHECK("bitnet_absmean_partial_kernel launch");
  ao::launch(bitnet_absmean_finish_kernel, dim3(1), dim3(kRowThreads), 0, (hipStream_t)stream, (const double*)workspace, blocks, numel, out, out_bf16);
  AO_LAUNCH_CHECK("bitnet_absmean_finish_kernel launch");
  return AO_OK;
}

extern "C" int ao_bitnet_quantize_weight(const uint16_t* w, const float* scale, uint8_t* packed, int8_t* q8, int64_t N, int64_t K, void* stream) {
  if (int rc = check_rows(__func__, N, K, 4)) return rc;
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(scale);
  AO_REQUIRE_PTR(packed);
  AO_REQUIRE(aligned_to(w, 16) && aligned_to(packed, 2) && aligned_to(q8, 8), "%s: w must be 16-byte, packed 2-byte and q8 8-byte aligned", __func__);
  const int64_t numel = N * K;
  ao::launch(bitnet_quantize_weight_kernel, dim3(grid_for((numel + 7) >> 3)), dim3(kRowThreads), 0, (hipStream_t)stream, w, scale, packed, q8, numel);
  AO_LAUNCH_CHECK("bitnet_quantize_weight_kernel launch");
  return AO_OK;
}

extern "C" int ao_bitnet_dequantize(const uint8_t* packed, uint16_t* out, int64_t N, int64_t K, void* stream) {
  if (int rc = check_rows(__func__, N, K, 4)) return rc;
  if (N == 0) return AO_OK;
  AO_REQUIRE_PTR(packed);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(packed, 4) && aligned_to(out, 16), "%s: packed must be 4-byte and out 16-byte aligned", __func__);
  const int64_t nbytes = N * (K / 4);
  ao::launch(bitnet_dequantize_kernel, dim3(grid_for(nbytes >> 2)), dim3(kRowThreads), 0, (hipStream_t)stream, packed, out, nbytes);
  AO_LAUNCH_CHECK("bitnet_dequantize_kernel launch");
  return AO_OK;
}

extern "C" int ao_bitnet_quantize_act(const uint16_t* x, int8_t* q, uint16_t* scale, int64_t M, int64_t K, void* stream) {
  if (int rc = check_rows(__func__, M, K, 8)) return rc;
  AO_REQUIRE(K <= (1ll << 24), "%s: K=%lld too large", __func__, (long long)K);
  if (M == 0) return AO_OK;
  AO_REQUIRE_PTR(x);
  AO_REQUIRE_PTR(q);
  AO_REQUIRE_PTR(scale);
  AO_REQUIRE(aligned_to(x, 16) && aligned_to(q, 8), "%s: x must be 16-byte and q 8-byte aligned", __func__);
  ao::launch(bitnet_quantize_act_kernel, dim3((unsigned)M), dim3(kRowThreads), 0, (hipStream_t)stream, x, q, scale, (int)K);
  AO_LAUNCH_CHECK("bitnet_quantize_act_kernel launch");
  return AO_OK;
}

extern "C" int ao_bitnet_mm_fits(int64_t M, int64_t N, int64_t K) { return bitnet_mm_check_shape(__func__, M, N, K) == AO_OK ? 1 : 0; }

extern "C" int ao_bitnet_mm(const int8_t* a, const uint8_t* w, const uint16_t* row_scale, const uint16_t* tensor_scale, const uint16_t* bias,
                            uint16_t* out, int64_t M, int64_t N, int64_t K, int form, void* stream) {
  if (int rc = bitnet_mm_check_shape(__func__, M, N, K)) return rc;
  AO_REQUIRE(form >= AO_BITNET_MM_AUTO && form <= AO_BITNET_MM_TILED, "%s: form=%d must be 0 (by M), 1 (streaming) or 2 (tiled)", __func__, form);
  if (M == 0 || N == 0) return AO_OK;
  AO_REQUIRE_PTR(a);
  AO_REQUIRE_PTR(w);
  AO_REQUIRE_PTR(row_scale);
  AO_REQUIRE_PTR(tensor_scale);
  AO_REQUIRE_PTR(out);
  AO_REQUIRE(aligned_to(a, 16) && aligned_to(w, 16) && aligned_to(out, 8), "%s: a and w must be 16-byte aligned and out 8-byte aligned", __func__);
  const BitnetMmArgs p{a, w, row_scale, tensor_scale, bias, out, (int)M, (int)N, (int)K};
  if (form == AO_BITNET_MM_AUTO) form = M <= AO_BITNET_MM_STREAM_MAX_M ? AO_BITNET_MM_STREAM : AO_BITNET_MM_TILED;
  if (form == AO_BITNET_MM_STREAM) {
    const size_t smem = kStreamRedBytes + (size_t)std::min<int64_t>(M, 16) * kStreamRowStride;  // at most 37120 bytes
    ao::launch(bitnet_mm_stream_kernel, dim3((unsigned)((N + 15) / 16), (unsigned)((M + 15) / 16)), dim3(256), smem, (hipStream_t)stream, p);
    AO_LAUNCH_CHECK("bitnet_mm_stream_kernel launch");
  } else {
    ao::launch(bitnet_mm_tile_kernel, dim3((unsigned)((N + kTileN - 1) / kTileN), (unsigned)((M + kTileM - 1) / kTileM)), dim3(256), 0,
               (hipStream_t)stream, p);
    AO_LAUNCH_CHECK("bitnet_mm_tile_kernel launch");
  }
  return AO_OK;
}
