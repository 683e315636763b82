// GPTQ for gfx950: the whole inner loop of ONE GPTQ block -- group qparams, quantize, dequantize, error, in-block propagation, final
// codes -- in ONE launch, the rows of the weight in parallel.
//
// Replaces the column loop of torchao/prototype/gptq/api.py:446-532 (and, for the block's columns, the final re-quantization :537-569),
// which the reference runs as eager ops on [N, 1] slices: about a dozen launches a column, tens of thousands a 4096 x 4096 weight.  The
// lazy batch update of the columns right of the block (:530-532) stays a torch matmul on the host (ao_amd/prototype/gptq/api.py).
//
// The arithmetic contract (restated in numpy by tests/gptq_ref.py; the bytes are the same): every operation is ONE fp32 operation rounded
// once; nothing is contracted into an fma (the reference's K = 1 matmul yields the rounded product, its subtraction rounds again); the
// divisions are IEEE; round is half-to-even; with bf16 weights every update of W rounds to bf16 (the reference's in-place `-=` on a bf16
// tensor with an fp32 right-hand side computes in fp32 and stores bf16).  For a block of columns [k0, k0 + bw) of W [N][K]:
//   for each quantization group that starts in the block: qparams from the CURRENT values of the group's columns, then frozen
//   for each column k of the group:   dq = dequantize(quantize(w));  err = (w - dq) / Hinv[k][k];
//                                     W[:, j] = round(W[:, j] - err Hinv[k][j]) for j = k .. k0 + bw - 1 (k itself included);  Err[:, k - k0] = err
//   the code of column k: quantize(its value after its own update) under the frozen qparams
// The formats:
//   int4 (zero-point flavour, api.py:167-221; qparams of mslk's int4_row_quantize_zp as include/ao_mi355.h states them for
//     ao_int4_plain_quantize):  scale = max(max - min, 1e-6) / 15;  zero = min + 8 scale  (int4_group_qparams, quant_math.h: the one
//     definition);  m = zero - 8 scale, which is this file's own and not always the group's min, so the code lines stay here too:
//     q = clamp(rint((w - m) / scale), 0, 15) - 8;  dq = (q + 8) scale + m.   PARITY UNPINNED: that the in-loop qparams stay fp32 (they are
//     rounded to the weight dtype only where they are stored) is this library's reading of the un-vendored mslk package.
//   NVFP4 (api.py:224-274; nvfp4_tensor.py:772-854), p the per-tensor scale:  s8 = e4m3(clamp((amax / 6) / p, 2^-6, 448));
//     r = (1 / p) / f32(s8);  c = e2m1(clamp(w r, -6, 6));  dq = f32(c) / r
//   int8 per row (int8_tensor.py:176-259), s the row's scale, given:  q = clamp(rint(w (1 / s)), -128, 127);  dq = q s
// NaN and Inf weights, and a zero or non-finite per-tensor scale, are outside the contract.
//
// Layout.  Step k needs row k of Hinv alone and the rows of W never meet, so a wave owns 16 rows for the whole block and needs no other
// wave: one wave a workgroup, no cross-wave barrier in the 256-step chain.  The wave's 64 lanes are 16 rows x 4 column parts: lane
// (r, p) updates the columns k + p, k + p + 4, ... of row r, so a row's update is spread over 4 lanes and N = 4096 gives 256 waves (one
// lane a row would give 64).  All 4 lanes of a row compute the same err from the same LDS word: redundant, bit-identical, and cheaper
// than a broadcast.  The tile lives in LDS as [column][row] with a row stride of 17 words: the 64 lanes of one update touch 4 columns
// x 16 rows = 64 different banks.  A 256 x 256 fp32 block of Hinv does not fit LDS: row k + 1 is fetched (one 16-byte load a lane) while
// step k runs and lands in the other half of a two-row LDS buffer.  (Fetching eight rows a batch ahead measured no faster -- a step waits
// on its own chain of LDS reads and divisions, not on memory -- and its 14 KiB of LDS cost a workgroup a CU at N = 14336.)  Err and the
// frozen qparams stay in LDS until the block is done and leave, with W and the codes, in one coalesced pass.  LDS: 17 KiB tile + 17 KiB
// Err + 2 KiB Hinv rows + 3 KiB qparams.
#include "common.h"
#include "quant_math.h"

namespace ao {
namespace {

constexpr int kRows = 16;        // rows of W a wave owns
constexpr int kParts = 4;        // lanes that share a row's columns
constexpr int kMaxBlock = 256;   // columns of one GPTQ block
constexpr int kStride = kRows + 1;
constexpr int kMaxGroups = kMaxBlock / 16;

enum Format { F_INT4 = AO_GPTQ_INT4, F_INT8 = AO_GPTQ_INT8, F_NVFP4 = AO_GPTQ_NVFP4 };

struct Args {
  void* W;
  const float* Hinv;
  float* Err;
  void* qdata;
  void* scale;        // int4: weight dtype [K/g][N];  NVFP4: e4m3 bytes [N][K/16]
  void* zero;         // int4: weight dtype [K/g][N]
  const float* aux;   // int8: fp32 [N] row scales;  NVFP4: the per-tensor scale
  int64_t N, K, k0;
  int bw, g;
};

// the frozen qparams of one group of one row: int4 (scale, m = zero - 8 scale) and zero for the store; NVFP4 (r, s8 bits); int8 (s, 1 / s)
struct QP {
  float a, b, z;
};

__device__ __forceinline__ float e2m1_value(uint32_t c) {
  const uint32_t e = (c >> 1) & 3u, man = c & 1u;
  const uint32_t mag = (e == 0u) ? (man ? 0x3f000000u : 0u) : (((e + 126u) << 23) | (man << 22));
  return bits_to_f32(mag | ((c & 8u) << 28));
}

template <int FMT>
__device__ __forceinline__ QP group_qparams(float mx, float mn, float p_or_s) {
#pragma clang fp contract(off)
  QP q;
  if (FMT == F_INT4) {
    int4_group_qparams(mx, mn, q.a, q.z);  // the shared (scale, zero)
    q.b = q.z - q.a * 8.0f;                // min_val = zero - scale * 8 (api.py:183, :217), not the group's min: GPTQ codes against its own m
  } else if (FMT == F_NVFP4) {
    const float amax = fmaxf(mx, -mn);
    const float bs = (amax / 6.0f) / p_or_s;
    const uint32_t s8 = cvt4_e4m3(fminf(fmaxf(bs, kE4M3Eps), 448.0f), 0.f, 0.f, 0.f) & 0xffu;
    q.a = (1.0f / p_or_s) / e4m3_byte_to_f32(s8);
    q.b = bits_to_f32(s8);
    q.z = 0.f;
  } else {
    q.a = p_or_s;
    q.b = 1.0f / p_or_s;
    q.z = 0.f;
  }
  return q;
}

// the code of one value (int4: q + 8 in 0..15; int8: q; NVFP4: the e2m1 code) and, in dq, what it dequantizes to
template <int FMT>
__device__ __forceinline__ int quantize(float w, const QP& q, float& dq) {
#pragma clang fp contract(off)
  if (FMT == F_INT4) {
    const float d = w - q.b;
    const float u = fminf(fmaxf(rintf(d / q.a), 0.f), 15.f);
    const float t = u * q.a;
    dq = t + q.b;
    return (int)u;
  } else if (FMT == F_NVFP4) {
    const float t = w * q.a;
    const uint32_t c = e2m1_code(f32_to_bits(clamp6(t)));
    dq = e2m1_value(c) / q.a;
    return (int)c;
  } else {
    const float t = w * q.b;
    const float u = fminf(fmaxf(rintf(t), -128.f), 127.f);
    dq = u * q.a;
    return (int)u;
  }
}

template <int FMT, bool BF16>
__global__ __launch_bounds__(kRows* kParts) void gptq_block_kernel(Args a) {
#pragma clang fp contract(off)
  __shared__ float tile[kMaxBlock * kStride];
  __shared__ float errs[kMaxBlock * kStride];
  __shared__ float hrow[2][kMaxBlock];
  __shared__ float qpa[kMaxGroups * kRows], qpb[kMaxGroups * kRows], qpz[kMaxGroups * kRows];

  const int lane = threadIdx.x, r = lane & (kRows - 1), p = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int bw = a.bw, g = a.g;
  const int64_t K = a.K, N = a.N, k0 = a.k0;
  const int rows = (int)((N - row0 < kRows) ? (N - row0) : kRows);

  // W[row0 .. row0 + 16)[k0 .. k0 + bw) -> tile[column][row]; rows past N hold zeros
  for (int idx = lane; idx < kRows * bw; idx += kRows * kParts) {
    const int rr = idx / bw, c = idx - rr * bw;
    float v = 0.f;
    if (rr < rows) {
      const int64_t at = (row0 + rr) * K + k0 + c;
      v = BF16 ? bf16_lo_to_f32(static_cast<const uint16_t*>(a.W)[at]) : static_cast<const float*>(a.W)[at];
    }
    tile[c * kStride + rr] = v;
  }
  const float* hbase = a.Hinv + k0 * K + k0;  // Hinv[k0 + k][k0 + j] = hbase[k K + j]
  if (lane * 4 < bw) {
    const f32x4 h = *reinterpret_cast<const f32x4*>(hbase + lane * 4);
    hrow[0][lane * 4 + 0] = h.x;
    hrow[0][lane * 4 + 1] = h.y;
    hrow[0][lane * 4 + 2] = h.z;
    hrow[0][lane * 4 + 3] = h.w;
  }
  float ps = 1.0f;  // NVFP4: the per-tensor scale;  int8: the row's scale (1 for the rows past N)
  if (FMT == F_NVFP4) ps = a.aux[0];
  if (FMT == F_INT8 && r < rows) ps = a.aux[row0 + r];

  QP qp = {1.f, 1.f, 0.f};
  for (int k = 0; k < bw; ++k) {
    __syncthreads();  // one wave: orders the LDS traffic of step k - 1 (tile, hrow) before step k
    f32x4 hn = {0.f, 0.f, 0.f, 0.f};
    const bool fetch = (k + 1 < bw) && (lane * 4 < bw);
    if (fetch) hn = *reinterpret_cast<const f32x4*>(hbase + (int64_t)(k + 1) * K + lane * 4);
    if (k % g == 0) {
      float mx = -INFINITY, mn = INFINITY;
      if (FMT != F_INT8) {
        for (int j = k + p; j < k + g; j += kParts) {
          const float v = tile[j * kStride + r];
          mx = fmaxf(mx, v);
          mn = fminf(mn, v);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mn = fminf(mn, __shfl_xor(mn, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        mn = fminf(mn, __shfl_xor(mn, 32));
      }
      qp = group_qparams<FMT>(mx, mn, ps);
      if (p == 0) {
        const int gi = k / g;
        qpa[gi * kRows + r] = qp.a;
        qpb[gi * kRows + r] = qp.b;
        qpz[gi * kRows + r] = qp.z;
      }
    }
    const float* h = hrow[k & 1];
    const float w = tile[k * kStride + r];
    float dq;
    quantize<FMT>(w, qp, dq);
    const float err = (w - dq) / h[k];
    if (p == 0) errs[k * kStride + r] = err;
#pragma unroll 8
    for (int j = k + p; j < bw; j += kParts) {
      const float prod = err * h[j];
      const float t = tile[j * kStride + r] - prod;
      tile[j * kStride + r] = BF16 ? round_bf16(t) : t;
    }
    if (fetch) {
      float* hw = hrow[(k + 1) & 1];
      hw[lane * 4 + 0] = hn.x;
      hw[lane * 4 + 1] = hn.y;
      hw[lane * 4 + 2] = hn.z;
      hw[lane * 4 + 3] = hn.w;
    }
  }
  __syncthreads();

  // every column is final: W, Err, the codes and the qparams leave
  for (int idx = lane; idx < kRows * bw; idx += kRows * kParts) {
    const int rr = idx / bw, c = idx - rr * bw;
    if (rr >= rows) continue;
    const float v = tile[c * kStride + rr];
    const int64_t at = (row0 + rr) * K + k0 + c;
    if (BF16)
      static_cast<uint16_t*>(a.W)[at] = f32_to_bf16_bits(v);
    else
      static_cast<float*>(a.W)[at] = v;
    a.Err[(row0 + rr) * bw + c] = errs[c * kStride + rr];
    if (FMT == F_INT8) {
      const QP q = {qpa[rr], qpb[rr], 0.f};
      float dq;
      static_cast<int8_t*>(a.qdata)[at] = (int8_t)quantize<FMT>(v, q, dq);
    }
  }
  if (FMT != F_INT8) {
    const int hb = bw / 2;
    for (int idx = lane; idx < kRows * hb; idx += kRows * kParts) {
      const int rr = idx / hb, b = idx - rr * hb;
      if (rr >= rows) continue;
      const int gi = (2 * b) / g;
      const QP q = {qpa[gi * kRows + rr], qpb[gi * kRows + rr], 0.f};
      float dq;
      int c0 = quantize<FMT>(tile[(2 * b) * kStride + rr], q, dq), c1 = quantize<FMT>(tile[(2 * b + 1) * kStride + rr], q, dq);
      if (FMT == F_INT4) {  // the signed code q - 8 as a nibble
        c0 = (c0 - 8) & 0xF;
        c1 = (c1 - 8) & 0xF;
      }
      static_cast<uint8_t*>(a.qdata)[(row0 + rr) * (K / 2) + k0 / 2 + b] = (uint8_t)(c0 | (c1 << 4));  // even k in the low nibble
    }
    const int groups = bw / g;
    for (int idx = lane; idx < groups * kRows; idx += kRows * kParts) {
      const int gi = idx / kRows, rr = idx - gi * kRows;
      if (rr >= rows) continue;
      if (FMT == F_INT4) {
        const int64_t at = (k0 / g + gi) * N + row0 + rr;
        if (BF16) {
          static_cast<uint16_t*>(a.scale)[at] = f32_to_bf16_bits(qpa[idx]);
          static_cast<uint16_t*>(a.zero)[at] = f32_to_bf16_bits(qpz[idx]);
        } else {
          static_cast<float*>(a.scale)[at] = qpa[idx];
          static_cast<float*>(a.zero)[at] = qpz[idx];
        }
      } else {
        static_cast<uint8_t*>(a.scale)[(row0 + rr) * (K / 16) + k0 / 16 + gi] = (uint8_t)f32_to_bits(qpb[idx]);
      }
    }
  }
}

template <int FMT>
int launch_gptq(const Args& a, bool bf16, hipStream_t s) {
  const int64_t blocks = (a.N + kRows - 1) / kRows;
  AO_REQUIRE(blocks < (1ll << 31), "ao_gptq_block: N=%lld is too large for one launch", (long long)a.N);
  dim3 grid((unsigned)blocks), block(kRows * kParts);
  if (bf16)
    ao::launch(gptq_block_kernel<FMT, true>, grid, block, 0, s, a);
  else
    ao::launch(gptq_block_kernel<FMT, false>, grid, block, 0, s, a);
  AO_LAUNCH_CHECK("gptq_block_kernel launch");
  return AO_OK;
}

}  // namespace
}  // namespace ao

using namespace ao;

extern "C" int ao_gptq_block(void* W, int w_bf16, const float* Hinv, float* Err, int format, int group_size, void* qdata, void* scale,
                             void* zero_point, const float* aux, int64_t N, int64_t K, int64_t k0, int64_t block_cols, void* stream) {
  AO_REQUIRE(format == AO_GPTQ_INT4 || format == AO_GPTQ_INT8 || format == AO_GPTQ_NVFP4, "ao_gptq_block: unknown format %d", format);
  AO_REQUIRE(N > 0 && K > 0, "ao_gptq_block: bad shape N=%lld K=%lld", (long long)N, (long long)K);
  AO_REQUIRE(block_cols > 0 && block_cols <= kMaxBlock, "ao_gptq_block: a GPTQ block holds 1 .. %d columns, got %lld (its tile of W and Err stay in LDS)",
             kMaxBlock, (long long)block_cols);
  int g = 16;  // the group the shape rules are checked against; int8 has none: the 16 of the kernel's 16-byte steps
  if (format == AO_GPTQ_INT4) {
    AO_REQUIRE(group_size == 32 || group_size == 64 || group_size == 128 || group_size == 256,
               "ao_gptq_block: int4 group_size must be one of 32, 64, 128, 256, got %d", group_size);
    g = group_size;
  } else if (format == AO_GPTQ_NVFP4) {
    AO_REQUIRE(group_size == 16, "ao_gptq_block: NVFP4 blocks hold 16 elements, got group_size %d", group_size);
    g = 16;
  }
  AO_REQUIRE(K % 16 == 0 && K % g == 0, "ao_gptq_block: K=%lld must be a multiple of 16 and of the group size %d", (long long)K, g);
  AO_REQUIRE(block_cols % 16 == 0 && block_cols % g == 0, "ao_gptq_block: the block's %lld columns must be a multiple of 16 and of the group size %d",
             (long long)block_cols, g);
  AO_REQUIRE(k0 >= 0 && k0 % 16 == 0 && k0 % g == 0 && k0 + block_cols <= K,
             "ao_gptq_block: the block [%lld, %lld) must start on a group and end inside K=%lld", (long long)k0, (long long)(k0 + block_cols),
             (long long)K);
  AO_REQUIRE_PTR(W);
  AO_REQUIRE_PTR(Hinv);
  AO_REQUIRE_PTR(Err);
  AO_REQUIRE_PTR(qdata);
  if (format != AO_GPTQ_INT8) AO_REQUIRE_PTR(scale);
  if (format == AO_GPTQ_INT4) AO_REQUIRE_PTR(zero_point);
  if (format != AO_GPTQ_INT4) AO_REQUIRE_PTR(aux);
  AO_REQUIRE(aligned_to(Hinv, 16), "ao_gptq_block: Hinv must be 16-byte aligned");
  // (int8: the kernel freezes its qparams -- the given row scale -- once, at the block's first column: one "group", the block)
  const Args a = {W, Hinv, Err, qdata, scale, zero_point, aux, N, K, k0, (int)block_cols, format == AO_GPTQ_INT8 ? (int)block_cols : g};
  hipStream_t s = (hipStream_t)stream;
  switch (format) {
    case AO_GPTQ_INT4: return launch_gptq<F_INT4>(a, w_bf16 != 0, s);
    case AO_GPTQ_INT8: return launch_gptq<F_INT8>(a, w_bf16 != 0, s);
    default: return launch_gptq<F_NVFP4>(a, w_bf16 != 0, s);
  }
}
