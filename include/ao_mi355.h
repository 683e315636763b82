/*
 * ao_mi355.h -- C ABI of the MI355X (gfx950) low-bit linear backend.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.  All
 * pointers are DEVICE pointers (HBM) unless a name ends in `_host`; `stream` is
 * a hipStream_t passed as void* (NULL = the default stream).  Every entry point
 * is asynchronous with respect to the host: it validates its arguments on the
 * host, enqueues kernels on `stream` and returns.  Inputs are borrowed and never
 * written; outputs must be caller-allocated (the Python host layer in
 * ao_amd/ops.py allocates them the way the reference ops allocate-and-return).
 *
 * Return value: AO_OK (0) or a negative AO_ERR_* code; ao_last_error() gives
 * the thread-local human readable message (the host layer raises RuntimeError /
 * ValueError from it, mirroring STD_TORCH_CHECK in
 * torchao/csrc/cuda/mx_kernels/mxfp8_extension.cpp:95-134).  The library never
 * calls exit().
 *
 * Library state: the only device memory the library owns is a split-K scratch
 * buffer per (device, stream) that launches split-K shapes (batched int4 on
 * narrow N, 8-bit linears with few output tiles).  It is allocated on that
 * stream's first such launch and grows in powers of two (8 MiB .. 128 MiB) to the
 * largest request seen on the stream; at most 8 streams per device hold one at a
 * time -- a ninth evicts the least recently used one after a device
 * synchronise.  Allocation, growth and eviction are impossible inside stream
 * capture: call the op once on the stream with its largest shape before
 * capturing, and re-capture graphs of a stream that lost its buffer.
 *
 * Each entry point cites the reference interface it replaces
 * (paths relative to the torchao checkout, lines from the 0.19.0 snapshot).
 * bf16 tensors are passed as uint16_t*, fp8 e4m3fn / e8m0 as uint8_t*.
 */
#ifndef AO_MI355_H
#define AO_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AO_OK 0
#define AO_ERR_INVALID_ARGUMENT (-1) /* shape / alignment / enum not supported */
#define AO_ERR_NULL_POINTER (-2)
#define AO_ERR_HIP (-3) /* a HIP runtime call failed; message has hipGetErrorString */

#define AO_MI355_ABI_VERSION 2 /* 2: ao_moe_a2a_v takes max_in_rows; peer memory + MAX all-reduce entry points */

/* Library / ABI version and last error of the calling thread. */
int ao_abi_version(void);
const char* ao_last_error(void);

/* Pre-size the split-K scratch buffer of `stream` (see "Library state" above) outside stream capture: afterwards every op on that stream is
 * capture-safe whatever its shape, without a warm-up call per shape.  bytes <= 0 reserves the cap (128 MiB); smaller requests are rounded up
 * to the next power of two >= 8 MiB.  The reference's ops own no workspace (SURVEY 8(b) "stateless"); its split-K lives inside hipBLASLt /
 * cuBLAS, which pre-allocate theirs per handle the same way (ATen's cublas workspace, CUDABlas / CublasHandlePool). */
int ao_splitk_reserve(void* stream, int64_t bytes);

/* Read-only view of the scratch buffer `stream` holds on the current device: allocates nothing, launches nothing and does not count as a use
 * of the buffer.  out_host[0] = 1 if the stream holds one (else 0), [1] = the capacity of its partial-tile area in bytes, [2] = its base
 * address (both 0 if none), [3] = the number of outgrown buffers the process keeps alive for graphs captured before a growth. */
int ao_splitk_query(void* stream, int64_t out_host[4]);

/* Per-launch kernel timing for benchmarks: after ao_prof_enable(n) the next n
 * kernel launches of this library are bracketed with HIP extension events that
 * timestamp the dispatch itself (begin/end of the kernel, no launch gaps).
 * ao_prof_collect() waits for them, writes the durations in milliseconds in
 * launch order to a HOST array and disables profiling.  Not thread-safe; do not
 * use during graph capture. */
int ao_prof_enable(int max_records);
int ao_prof_collect(float* ms_out_host, int capacity, int* n_out_host);

/* ------------------------------------------------------------------------- *
 * int4 weight-only, tinygemm "tile packed to 4d" format
 * ------------------------------------------------------------------------- */

/* Replaces aten::_convert_weight_to_int4pack(Tensor self, int innerKTiles) as
 * called at torchao/quantization/quantize_/workflows/int4/
 * int4_tile_packed_to_4d_tensor.py:202.
 *   w_u8   uint8 [N][K/2], even k in the high nibble (:199-201)
 *   qdata  int32 [N/8][K/(inner_k_tiles*16)][32][inner_k_tiles/2], gfx950 tile
 *          order (one wavefront owns a 16(n) x 128(k) tile)
 * Requires N % 16 == 0, K % (inner_k_tiles*16) == 0, inner_k_tiles == 8. */
int ao_int4_convert_weight_to_int4pack(const uint8_t* w_u8, int32_t* qdata,
                                       int64_t N, int64_t K, int inner_k_tiles,
                                       void* stream);

/* Inverse of the above (bit-exact): qdata -> uint8 [N][K/2].  Used by
 * Int4TilePackedTo4dTensor.dequantize()/slicing tests; no reference op
 * (the reference unpacks by multiplying with an identity matrix,
 * torchao/quantization/utils.py:198-226). */
int ao_int4_unpack_int4pack(const int32_t* qdata, uint8_t* w_u8, int64_t N,
                            int64_t K, int inner_k_tiles, void* stream);

/* Replaces aten::_weight_int4pack_mm(Tensor self, Tensor mat2, int qGroupSize,
 * Tensor qScaleAndZeros) as called at int4_tile_packed_to_4d_tensor.py:287.
 *   x               bf16 [M][K]
 *   qdata           int32 4-D as above (N x K logical)
 *   scale_and_zero  bf16 [K/group_size][N][2]   (torchao/quantization/utils.py:299-313)
 *   y               bf16 [M][N]
 * y[m][n] = sum_k x[m][k] * bf16(bf16((q[n][k]-8) * s[k/g][n]) + z[k/g][n]),
 * fp32 accumulation (the dequant->bf16-matmul oracle, quant_primitives.py:999-1007).
 * group_size in {32, 64, 128, 256}; N % 16 == 0; K % 128 == 0; K % group_size == 0. */
int ao_int4_weight_int4pack_mm(const uint16_t* x, const int32_t* qdata,
                               const uint16_t* scale_and_zero, uint16_t* y,
                               int64_t M, int64_t N, int64_t K, int group_size,
                               void* stream);

/* Two aten::_weight_int4pack_mm calls of one M, N, K and group size in one launch (call site: int4_tile_packed_to_4d_tensor.py:287,
 * reached twice in a row by modules that keep twin linears apart -- gate_proj / up_proj, k_proj / v_proj -- on the same activation).
 * Arguments and requirements per problem as for ao_int4_weight_int4pack_mm; x0 == x1 is allowed, the weights are only read.
 * Returns AO_OK with y0, y1 holding, bit for bit, what the two single calls store.  Where the problem's route is a one-row (M = 1)
 * straight-line form of int4_mm_kernel and ao_int4_pair_independent holds, that is ONE launch of int4_mm_pair_kernel (grid.z = 2);
 * on every other route, or when the second problem depends on the first, the entry makes the two single launches in order
 * (problem 0 first) -- it never fails because the pair form does not apply. */
int ao_int4_weight_int4pack_mm_pair(const uint16_t* x0, const int32_t* qdata0, const uint16_t* scale_and_zero0, uint16_t* y0,
                                    const uint16_t* x1, const int32_t* qdata1, const uint16_t* scale_and_zero1, uint16_t* y1,
                                    int64_t M, int64_t N, int64_t K, int group_size, void* stream);
/* The pair's independence rule, host arithmetic on addresses only: 1 when [y1, y1 + M N) overlaps neither [x0, x0 + M K) nor
 * [y0, y0 + M N) and [x1, x1 + M K) does not overlap [y0, y0 + M N) (elements of 2 bytes), else 0. */
int ao_int4_pair_independent(const uint16_t* x0, const uint16_t* y0, const uint16_t* x1, const uint16_t* y1, int64_t M, int64_t N,
                             int64_t K);
/* How many times ao_int4_weight_int4pack_mm, called under stream capture, folded its launch into the kernel node of the call before it
 * ("twin linears"): a running count of the process (saturates at INT_MAX).  Host only. */
int ao_int4_pair_fusions(void);

/* Dequantize the packed weight to bf16 [N][K] with the oracle's rounding
 * sequence.  Replaces groupwise_affine_dequantize_tensor
 * (torchao/quantization/utils.py:445-455) for the packed format. */
int ao_int4_dequantize(const int32_t* qdata, const uint16_t* scale_and_zero,
                       uint16_t* w_bf16, int64_t N, int64_t K, int group_size,
                       void* stream);

/* Fused weight preparation: _choose_qparams_affine_tinygemm +
 * _quantize_affine_tinygemm + nibble pack + _convert_weight_to_int4pack +
 * pack_tinygemm_scales_and_zeros (int4_tile_packed_to_4d_tensor.py:129-236,
 * quant_primitives.py:1299-1335,577-599; utils.py:299-313) in one pass.
 *   w  bf16 [N][K] (already padded: N % 16 == 0, K % 128 == 0, K % g == 0). */
int ao_int4_quantize_tinygemm(const uint16_t* w, int32_t* qdata,
                              uint16_t* scale_and_zero, int64_t N, int64_t K,
                              int group_size, void* stream);

/* Launch-shape override for tuning sweeps (bench/tools only): waves per
 * workgroup (0 = heuristic) and an A/B mode of the int4 mm (0 = product dispatch).  Every mode this library honours computes the
 * SAME result as the product (other ring depths, tile shapes, K splits, trace stamps); the ablation builds that drop parts of the
 * kernel -- and so return wrong numbers -- exist only in the laboratory build (`python -m ao_amd.build --lab` ->
 * tools/bin/_C_mi355_lab.so, compiled with -DAO_LAB; tools select it through AO_MI355_LIB).  Thread-local.
 * Modes 981 - 984 steer only the balanced grid of the one-row kernel and leave every other choice the product's: 981 never,
 * 982 wherever the form allows (one row, K = 4096: any left-over tile count, for A/B and tests on small shapes), 983 / 984 the stamped
 * profiling build (g = 128; [workgroups][8] u64 into the ao_int4_set_trace buffer) on today's grid / on the grid of 982.
 * Modes 985 / 986 steer only the twin-linear pair: 985 never fuse two captured calls into one node, 986 the pair grid
 * with each problem's balanced halves (the product pair runs one workgroup per tile; A/B). */
int ao_int4_set_tuning(int waves_per_block, int mode);
/* 1 when the calling thread has an ao_int4_set_tuning override set, else 0 (tests assert the product dispatch).  Host only. */
int ao_int4_overridden(void);
/* Profiling only: 0 = product dispatch of the 8-bit GEMMs (LDS-DMA staged kernel when K % 128 == 0),
 * 1 = force the register-staged kernel, 2 / 4 / 8 = force the LDS-DMA kernel with 128x128, 256x128 (4 waves), 256x256 (8 waves) tiles,
 * 32 = the phase-interleaved 256x256 kernel, 33 = its 256x128 form (gemm8_p8h_kernel); 100 / 101 / 102 = the fp8 weight-streaming kernel never / always / always with 64-column tiles; 103 = its round-3 wave arrangement (1 x 8);
 * MXFP8 grouped mm: 111 never the LDS-staged kernels (A-stationary / per-tile kernels), 110 the product route (kept so old scripts run); decode-size groups: 113 one workgroup
 * per tile instead of the stream-K kernel, 129 the stream-K kernel's per-step-scales form (what K % 512 != 0 takes) on every K
 * (ao_amd/csrc/rb8_kernels.hip); the decode kernel (dec8_kernel): 201 .. 208 its ring depth, 290 half-line loads, 291 / 292 never /
 * always 8-row tiles, 293 the round-4 bound of 64 KiB of activation codes (product since round 6: the CU's whole LDS), 299 never;
 * 300 / 301 / 31S the register-ring mid-M kernel never / wherever the shape allows / with S K parts.  Thread-local, like ao_int4_set_tuning. */
int ao_gemm8_set_variant(int variant);
/* Profiling only, key / value (every setting computes the SAME result as the product; 0 = product rule; thread-local):
 *   key 1  column-tile width of the rowwise weight-streaming kernel (rb8_kernel): 32, 64 or 128
 *   key 2  its K parts (1 .. 16)
 *   key 3  slab rows of rb8_kernel: 64 or 128 at any M (product: the cost model's pick above 64 rows, 64 up to 64)
 *   key 4  tile rows an XCD's workgroups of gemm8_p8_kernel walk together (product: 4)
 *   key 5  timing probes of the TRACED build of rb8_kernel only (ao_int4_set_trace set; results are wrong): bit 0 no MFMAs, 1 no fragment
 *          reads, 2 no weight DMAs, 3 no activation DMAs, 4 DMA wait + barrier on even steps only -- the product build ignores it
 *   key 6  the persistent form of the 256 x 256 GEMM (gemm8_p8p_kernel): 1 never, 2 wherever the shape allows
 *   key 7  K parts of gemm8_p8h_kernel (1 .. 16, clamped to what fits one round of the chip and the split-K workspace)
 *   key 8  retired (it chose among laboratory loop forms of gemm8_p8h_kernel, profiles/p8h_loop_forms_r05.jsonl): accepted so that old
 *          scripts run, sets nothing, and does not make ao_gemm8_overridden() report an override
 *   key 9  the MXFP8 stream-K kernel's meeting, A/B: bit 0 the head piece's ticket after the loop, bit 1 no early read of the tail ticket
 *          (3 = the round-3 protocol)
 * An unknown key is an error.  DESIGN.md 4.5h. */
int ao_gemm8_set_tuning(int key, int value);
/* 1 when the calling thread has any ao_gemm8_set_variant / ao_gemm8_set_tuning override set, else 0.  Host only. */
int ao_gemm8_overridden(void);
/* Name of the kernel ao_int4_weight_int4pack_mm launches for this problem: the product route, whatever override
 * ao_int4_set_tuning has set -- what a profiler's kernel table should be matched against.  Static string. */
const char* ao_int4_mm_kernel_name(int64_t M, int64_t N, int64_t K, int group_size);
/* Every field of that product route (host logic only): out[cap >= 10] = form (0 int4_mm_kernel, 1 int4_mm_rb_kernel, 2 int4_mm_w32_kernel),
 * rows of the per-tile build, ring depth, straight-line, waves, n-tiles, m-tiles, column groups (w32: 2 = 128 x 256 tiles), K parts,
 * producer form.  With cap >= 11 also out[10] = the n-tiles the one-row kernel runs as two half-tile workgroups each (the balanced grid;
 * 0 = one workgroup per tile; K parts stays 1). */
int ao_int4_mm_route(int64_t M, int64_t N, int64_t K, int group_size, int32_t* out, int cap);
/* The balanced grid's rule, host arithmetic only: of `tiles` n-tiles on `cus` compute units, how many the one-row kernel cuts in two
 * (r = tiles mod cus when cus < tiles <= 4 cus and 2 r = cus, else 0; forced != 0, the rule of tuning mode 982: r whatever it is). */
int ao_int4_balanced_halves(int64_t tiles, int cus, int forced);
/* Which kernel ao_fp8_scaled_mm (int8 = 0) / ao_int8_scaled_mm (int8 = 1) dispatches a shape to: "dec8_kernel" (M <= 16), "mid8_kernel",
 * "stream8_kernel", "rb8_kernel" (up to 256 tiles of 128 x 128), "gemm8_p8h_kernel" / "gemm8_p8_kernel" / "gemm8_p8p_kernel" /
 * "gemm8_dma_kernel<...>" / "gemm8_kernel" (tiled), or "invalid".  The route the launch takes for 16-byte-aligned scales and output, whatever
 * override ao_gemm8_set_variant / ao_gemm8_set_tuning has set (the product dispatch).  Host logic only (no launch): bench / tests label their
 * measurements with it.  DESIGN.md 4.4-4.5g. */
const char* ao_gemm8_kernel_name(int int8, int64_t M, int64_t N, int64_t K);
/* The launch shape of that same route: column-tile width and K parts (rb8_kernel: the cost model's pick; gemm8_p8h_kernel: 128 columns and
 * 1 .. 4 parts; the per-tile streaming kernels: 16, one part; others: their tile width, one part).  Host logic only.  DESIGN.md 4.5h. */
int ao_gemm8_plan(int int8, int64_t M, int64_t N, int64_t K, int* tile_cols, int* k_parts);
/* The rows of that route's tile: rb8_kernel's slab height (64 up to 64 rows; 64 or 128 beyond, by the cost model -- round 6: 64-row slabs
 * cut M instead of K where the fixed costs of a launch outweigh its loop), 256 for the 256 x 128 / 256 x 256 GEMMs, 128 / 16 otherwise.
 * Host logic only.  DESIGN.md 4.5. */
int ao_gemm8_plan_rows(int int8, int64_t M, int64_t N, int64_t K, int* tile_rows);
/* Every field of the product route of one 8-bit entry point, for aligned (1) or unaligned (0) scales / bias (the route the launch takes
 * with no override set; host logic only).  entry: 0 ao_int8_scaled_mm, 1 ao_fp8_scaled_mm, 2 ao_int8_int_mm, 3 ao_fp8_mm_f32,
 * 4 ao_int8_dynamic_linear, 5 ao_fp8_dynamic_linear.  out[cap >= 11] = kernel (0 = invalid, then the ao_gemm8_kernel_name order: dec8,
 * mid8, stream8, rb8, p8h, p8, p8p, dma 128x128, dma 256x256, dma 256x128, dma 256x256 4 waves, gemm8_kernel, dyn8), tile rows,
 * tile columns, K parts, dec8 waves, depth, loop, half, rows8, mid8 m-tiles, mid8 K parts. */
int ao_gemm8_route(int entry, int64_t M, int64_t N, int64_t K, int aligned, int32_t* out, int cap);
/* Every field of the product route of one grouped entry point (host logic only; offs given; the fused cast as AO_MX_SCALE_RCEIL), for
 * aligned (1) or unaligned (0) operands -- the scales, and the activations of the fused-cast and pair forms.  entry: 0 ao_fp8_grouped_mm,
 * 1 ao_mxfp8_grouped_mm, 2 ao_mxfp8_grouped_mm_dyn, 3 ao_mxfp8_grouped_mm_dyn_pair, 4 ao_mxfp8_grouped_mm_pair.  out[cap >= 10] = kernel
 * (0 = invalid: the entry refuses the shape, 1 rb8_kernel, 2 mx_stream_kernel, 3 mx_grouped_kernel, 4 stream8_kernel), waves, m-tiles,
 * slim, scale fetches per 1 / 4 k steps, weight stages, cast (0 none, 1 floor, 2 rceil), n-tiles, slab rows, slabs per group. */
int ao_grouped8_route(int entry, int64_t M_total, int64_t N, int64_t K, int64_t E, int aligned, int32_t* out, int cap);
/* Which form of fp8_int4_mm_kernel ao_fp8_int4_linear launches for a shape: "<m-tiles x n-tiles>" of 16 x 16 per workgroup -- "<1x1>" up to
 * 16 rows, "<2x1>" / "<2x2>" beyond (round 5: the weights stream once per 32 rows, the staged activations serve 32 columns), or "invalid".
 * Host logic only.  DESIGN.md 4.9. */
const char* ao_fp8_int4_kernel_name(int64_t M, int64_t N, int64_t K, int group_size);
/* Profiling only: device buffer [workgroups][16] of s_memtime stamps written by the trace builds of the batched
 * kernels (int4: tuning mode 65S; fp8 rowwise mid-M kernel: whenever the pointer is set); NULL disables.  The stamped one-row int4
 * build (tuning modes 983 / 984) writes [workgroups][8] instead. */
int ao_int4_set_trace(unsigned long long* trace_dev);

/* ------------------------------------------------------------------------- *
 * int8 dynamic activation x int8 weight
 * ------------------------------------------------------------------------- */

/* Per-row symmetric int8 quantization of a bf16 matrix: replaces
 * Int8Tensor.from_hp(x, PerRow) = choose_qparams_affine(SYMMETRIC, eps=fp32 eps)
 * + quantize_affine (torchao/quantization/quantize_/workflows/int8/
 * int8_tensor.py:176-248; quant_primitives.py:1534-1583,463-485).
 *   x bf16 [M][K] -> q int8 [M][K], scale fp32 [M] */
int ao_int8_quantize_rowwise(const uint16_t* x, int8_t* q, float* scale,
                             int64_t M, int64_t K, void* stream);

/* Replaces _int_scaled_matmul/safe_int_mm -> aten::_int_mm plus the scale
 * epilogue of the Int8Tensor linear (int8/kernels.py:114-144, int8_tensor.py:
 * 315-359):  y = bf16( bf16( (xq @ wq^T)_i32 * x_scale[m] ) * w_scale[n] ) (+bias).
 *   xq int8 [M][K]; wq int8 [N][K] (row-major weight, i.e. the reference's
 *   weight.qdata before its .contiguous().t()); x_scale fp32 [M];
 *   w_scale fp32 [N]; bias bf16 [N] or NULL; y bf16 [M][N].  K % 16 == 0. */
int ao_int8_scaled_mm(const int8_t* xq, const float* x_scale, const int8_t* wq,
                      const float* w_scale, const uint16_t* bias, uint16_t* y,
                      int64_t M, int64_t N, int64_t K, void* stream);

/* Plain aten::_int_mm (int8/kernels.py:38-40,70): c int32 [M][N] = a[M][K] @ b_t[N][K]^T. */
int ao_int8_int_mm(const int8_t* a, const int8_t* b_t, int32_t* c, int64_t M,
                   int64_t N, int64_t K, void* stream);

/* Asymmetric per-row activation quantization: Int8Tensor.from_hp(x, PerRow(), mapping_type=ASYMMETRIC), the activation side
 * of Int8DynamicActivationInt8WeightConfig(act_mapping_type=ASYMMETRIC) (int8_tensor.py:191-236; choose_qparams_affine's
 * ASYMMETRIC branch quant_primitives.py:1568-1574; quantize_affine :463-485), bf16 input:
 *   mn = min(row, 0), mx = max(row, 0); scale = max(bf16(bf16(mx - mn) / 255), f32_eps);
 *   zero_point = clamp(-128 - rint(bf16(mn / scale)), -128, 127); q = clamp(rint(x / scale) + zero_point, -128, 127)
 *   x bf16 [M][K] -> q int8 [M][K], scale fp32 [M], zero_point int8 [M] */
int ao_int8_quantize_rowwise_asym(const uint16_t* x, int8_t* q, float* scale, int8_t* zero_point,
                                  int64_t M, int64_t K, void* stream);
/* Static activation quantization: Int8Tensor.from_hp(x, granularity, mapping_type, scale=..., zero_point=...) with the qparams GIVEN
 * (Int8StaticActivationInt8WeightConfig, quant_api.py:919-1012; int8_tensor.py:212-231): q = clamp(rint(x / scale) + zp, -128, 127).
 *   x bf16 [M][K]; scale fp32 [1] (per_row = 0) or [M] (per_row = 1); zero_point int8, same shape, or NULL (symmetric) -> q int8 [M][K] */
int ao_int8_quantize_static(const uint16_t* x, const float* scale, const int8_t* zero_point, int per_row,
                            int8_t* q, int64_t M, int64_t K, void* stream);
/* rowsum(W_int8) of the zero-point correction (int8_tensor.py:326 `weight_tensor.qdata.sum(dim=-1)`): q int8 [N][K] ->
 * sums int32 [N].  K % 16 == 0.  Computed once per weight by the host mirror. */
int ao_int8_row_sums(const int8_t* q, int32_t* sums, int64_t N, int64_t K, void* stream);
/* The Int8Tensor linear's epilogue with an asymmetric activation (int8_tensor.py:305-346) over the int32 accumulator of
 * ao_int8_int_mm:  t = bf16(f32(acc) * x_scale[m]);  t = bf16(t - bf16((zp[m] * x_scale[m]) * w_row_sums[n]));
 *   y = bf16(t * w_scale[n] (+ bias[n])). */
int ao_int8_scale_epilogue_asym(const int32_t* acc, const float* x_scale, const int8_t* x_zero_point,
                                const int32_t* w_row_sums, const float* w_scale, const uint16_t* bias,
                                uint16_t* y, int64_t M, int64_t N, void* stream);

/* ------------------------------------------------------------------------- *
 * float8 (OCP e4m3fn) rowwise
 * ------------------------------------------------------------------------- */

/* Replaces Float8Tensor.from_hp(x, e4m3, PerRow): _choose_scale_float8 +
 * _quantize_affine_float8 (float8_tensor.py:167-253; quant_primitives.py:
 * 2172-2212,2271-2287): scale[r] = f32(bf16(amax_r / 448)), q = e4m3(clamp(x/scale)).
 *   x bf16 [M][K] -> q e4m3fn [M][K], scale fp32 [M] */
int ao_fp8_quantize_rowwise(const uint16_t* x, uint8_t* q, float* scale,
                            int64_t M, int64_t K, void* stream);

/* Replaces aten::_scaled_mm with rowwise scales as called from
 * addmm_float8_unwrapped_inference (torchao/float8/inference.py:86-123):
 *   y = bf16( (a @ b^T)_f32 * scale_a[m] * scale_b[n] + bias[n] )
 *   a e4m3fn [M][K] row-major; b e4m3fn [N][K] row-major (== the reference's
 *   column-major [K][N] mat2); scale_a fp32 [M]; scale_b fp32 [N];
 *   bias bf16 [N] or NULL; y bf16 [M][N].  K % 16 == 0, N % 16 == 0. */
int ao_fp8_scaled_mm(const uint8_t* a, const uint8_t* b, const float* scale_a,
                     const float* scale_b, const uint16_t* bias, uint16_t* y,
                     int64_t M, int64_t N, int64_t K, void* stream);

/* ---- float8 TRAINING casts (torchao.float8: hp_tensor_to_float8_dynamic, float8_scaling_utils.py:29-72) --------------------------
 * Not the arithmetic of ao_fp8_quantize_rowwise:
 *   scale = f32(448 / max(f64(amax), 1e-12))                                  (float8_utils.py:31-53: a float64 division)
 *   pow2 != 0: scale = exp2(floor(log2(scale))), the mantissa bits cleared     (float8_utils.py:244-246)
 *   q = e4m3fn_rne(clamp(f32(x) * scale, -448, 448))                           (float8_training_tensor.py:153-154, float8_utils.py:118-139)
 *   inv_scale = 1.0f / scale, what ao_fp8_scaled_mm multiplies by              (float8_ops.py:44-45)
 * x bf16 [R][C], finite.  C % 16 == 0; R % 16 == 0 where a transposed output is asked for; R == 0 or C == 0 launches nothing.  No
 * allocation, no synchronisation: capturable in a graph. */

/* tensor_to_amax (float8_utils.py:56-82) along either or both axes in ONE read of x: row_amax fp32 [R] = max |x| over each row
 * (axiswise_dim = -1), col_amax fp32 [C] = over each column (axiswise_dim = 0); either may be NULL.  The tiles' partial maxima merge by an
 * atomic max into the outputs, which the call zeroes on `stream` first: the result does not depend on scheduling. */
int ao_fp8_train_amax(const uint16_t* x, float* row_amax, float* col_amax, int64_t R, int64_t C, void* stream);

/* hp_tensor_and_scale_to_float8 (float8_training_tensor.py:130-188) for either or both directions in ONE read of x:
 *   q_row e4m3fn [R][C], s_row / inv_s_row fp32 [R]       from row_amax  (the cast with axiswise_dim = -1)
 *   q_col_t e4m3fn [C][R], s_col / inv_s_col fp32 [C]     from col_amax  (the cast with axiswise_dim = 0, stored transposed: the
 *                                                          K-contiguous operand ao_fp8_scaled_mm takes for dgrad and wgrad)
 * q_row == NULL or q_col_t == NULL skips that direction.  An amax stride is 1, or 0 for ONE amax of the whole tensor (TENSORWISE
 * granularity; the scale vectors are then filled with the one scale, float8_ops.py:356-359). */
int ao_fp8_train_cast(const uint16_t* x, const float* row_amax, int64_t row_amax_stride, const float* col_amax,
                      int64_t col_amax_stride, int pow2, uint8_t* q_row, float* s_row, float* inv_s_row,
                      uint8_t* q_col_t, float* s_col, float* inv_s_col, int64_t R, int64_t C, void* stream);

/* The row direction alone (tensor_to_scale + hp_tensor_and_scale_to_float8 with axiswise_dim = -1, float8_scaling_utils.py:56-72) as ONE
 * launch: the bytes of ao_fp8_train_amax + ao_fp8_train_cast. */
int ao_fp8_train_quantize_rowwise(const uint16_t* x, uint8_t* q, float* s, float* inv_s, int pow2, int64_t R, int64_t C,
                                  void* stream);

/* ---- float8 rowwise training of the MoE grouped GEMM (torchao/prototype/moe_training/fp8_grouped_mm.py:24-319) -----------------------
 * The casts use the arithmetic above (scale, pow2, q, inv_scale).  No allocation, no synchronisation: capturable in a graph. */

/* The jagged column cast (kernels/jagged_float8_scales.py:221-252, utils.py:20-86 torch_to_float8_per_group_colwise): one scale per column
 * and token group.  x bf16 [R][C]; offs int32 [E] on the device, cumulative group ends along R ->
 *   q_t e4m3fn [C][R] (tokens innermost, as ao_fp8_train_cast's q_col_t), s / inv_s fp32 [E][C] (group-major: the reference's [E C] vector)
 * The amax of column c in group e runs over rows [offs[e-1], offs[e]).  An empty group gets the scale of a zero amax (448 / 1e-12) and its
 * reciprocal; rows at or past offs[E-1] belong to no group and get code 0.
 * offs is not validated.  Its contract: non-decreasing, within [0, R], every end a multiple of 16.  For any other int32 contents the
 * kernels stay inside their buffers and the values are unspecified.
 * R % 16 == 0, C % 16 == 0, 1 <= E <= 65535, R <= 65535 * 128; R == 0 or C == 0 launches nothing.  x, q_t, s 16-byte aligned.
 * Launches: a memset of s, the maxima (atomic max into s), the scales in place, the codes. */
int ao_fp8_train_quantize_group_colwise_t(const uint16_t* x, const int32_t* offs, uint8_t* q_t, float* s, float* inv_s, int pow2,
                                          int64_t R, int64_t C, int64_t E, void* stream);

/* The batched transposing cast of a 3-D weight (kernels/float8_rowwise.py, utils.py:156-189 torch_to_3d_rowwise_float8_transpose_rhs):
 * w bf16 [E][R][C] -> q_t e4m3fn [E][C][R], s / inv_s fp32 [E][C]; the amax along R, per expert.  Expert e's output is byte for byte that
 * of ao_fp8_train_amax(cols) + ao_fp8_train_cast(q_col_t) on w[e].  R % 16 == 0, C % 16 == 0, E <= 65535 and E * R <= 65535 * 128 (the
 * walk is over the [E R][C] view, 128 rows a tile; every index is 64-bit); E, R or C == 0 launches nothing. */
int ao_fp8_train_quantize_colwise_t_3d(const uint16_t* w, uint8_t* q_t, float* s, float* inv_s, int pow2, int64_t E, int64_t R,
                                       int64_t C, void* stream);

/* The weight gradient of the float8 rowwise grouped GEMM (fp8_grouped_mm.py:282-319: torch._scaled_grouped_mm, 2-D x 2-D with offsets) on
 * the two jagged casts:
 *   out[e][n][k] = bf16( (sum_{m in [offs[e-1], offs[e])} g_t[n][m] * x_t[k][m]) * g_inv[e][n] * x_inv[e][k] )
 * fp32 accumulation, one rounding.  offs == NULL (E == 1): one group of every token.  Any offsets (clamped to [0, M_total]); an empty group
 * stores zeros; tokens past offs[E-1] contribute to nothing.  M_total, N, K multiples of 16; E <= 65535; N * M_total and K * M_total below
 * 2^31 (32-bit buffer offsets); the codes 16-byte aligned.  M_total == 0 zeroes out. */
int ao_fp8_grouped_mm_wgrad(const uint8_t* g_t, const float* g_inv,   /* e4m3 [N][M_total], fp32 [E][N] */
                            const uint8_t* x_t, const float* x_inv,   /* e4m3 [K][M_total], fp32 [E][K] */
                            const int32_t* offs, uint16_t* out,       /* int32 [E], bf16 [E][N][K] */
                            int64_t M_total, int64_t N, int64_t K, int64_t E, void* stream);

/* HQQ qparams + codes for the tinygemm format: Int4TilePackedTo4dTensor.from_hp(..., HQQ)
 * (int4_tile_packed_to_4d_tensor.py:149-168 -> quant_primitives.py:1891-1997, optimizer :1797-1866 in float16 as on a GPU).
 *   w bf16 [N][K] -> nibble_bytes uint8 [N][K/2] (even k in the HIGH nibble: the input of
 *   ao_int4_convert_weight_to_int4pack), scale_and_zero bf16 [K/g][N][2].
 *   workspace: ao_int4_hqq_workspace_bytes(N, K, g) device bytes.  Host-synchronous like the reference: the optimizer's
 *   early stop reads a global error every iteration (<= 20 stream synchronisations); not capturable in a graph. */
int64_t ao_int4_hqq_workspace_bytes(int64_t N, int64_t K, int group_size);
int ao_int4_quantize_hqq(const uint16_t* w, uint8_t* nibble_bytes, uint16_t* scale_and_zero, void* workspace,
                         int64_t N, int64_t K, int group_size, void* stream);

/* Int4Tensor.from_hp, PLAIN packing (quantize_/workflows/int4/int4_tensor.py:130-186): the arithmetic of mslk's
 * int4_row_quantize_zp / int4_row_quantize + pack_int4 (un-vendored; restated by the reference at
 * quantization/qat/fake_quantizer.py:148-190 and prototype/gptq/api.py:167-221), fp32 math:
 *   symmetric = 0: scale = max(max - min, 1e-6) / 15, zero = min + 8 scale, q = clamp(rint((w - min) / scale), 0, 15) - 8
 *   symmetric = 1: scale = max(max|w| / 8, 1e-6), zero = 0, q = clamp(rint(w / scale), -8, 7)   (fp8-activation flavour)
 *   w bf16 [N][K] -> qdata uint8 [N][K/2] (even k in the LOW nibble), scale / zero_point bf16 [K/g][N]. */
int ao_int4_plain_quantize(const uint16_t* w, uint8_t* qdata, uint16_t* scale, uint16_t* zero_point,
                           int64_t N, int64_t K, int group_size, int symmetric, void* stream);

/* ------------------------------------------------------------------------- *
 * MXFP8 (e4m3 elements, E8M0 scale per 32 along the contraction dim)
 * ------------------------------------------------------------------------- */

#define AO_MX_SCALE_FLOOR 0
#define AO_MX_SCALE_RCEIL 1

/* Replaces torchao::mxfp8_quantize (rowwise 1x32 cast; schema
 * torchao/prototype/mx_formats/kernels.py:1022-1026; semantics to_mx,
 * torchao/prototype/mx_formats/mx_tensor.py:228-409).
 *   x bf16 [R][C] (C % 32 == 0) -> q e4m3fn [R][C], scale e8m0 [R][C/32]. */
int ao_mxfp8_quantize_rowwise(const uint16_t* x, uint8_t* q, uint8_t* scale_e8m0,
                              int64_t R, int64_t C, int scaling_mode,
                              void* stream);

/* The colwise half of torchao::mxfp8_quantize (32 x 1 blocks: one scale per 32 ROWS of a column;
 * csrc/cuda/mx_kernels/mxfp8_quantize.cuh:460-820, mxfp8_extension.cpp:160-175; == to_mx(x.t()).t()).
 *   x bf16 [R][C] (R % 32 == 0, C % 32 == 0) -> q_t e4m3fn [C][R] (the column-major data the reference
 *   returns as a {R, C} tensor with strides {1, R}), scale e8m0 [R/32][C] (its {C, R/32} tensor with strides {1, C}). */
int ao_mxfp8_quantize_colwise(const uint16_t* x, uint8_t* q_t, uint8_t* scale_e8m0,
                              int64_t R, int64_t C, int scaling_mode, void* stream);

/* torchao::mxfp8_quantize with rowwise AND colwise set, in one launch that reads x once (the reference's CUDA kernel does the same,
 * mxfp8_quantize.cuh:460-820): q_row / s_row hold exactly the bytes of ao_mxfp8_quantize_rowwise, q_col_t / s_col exactly those of
 * ao_mxfp8_quantize_colwise.  x bf16 [R][C], R % 32 == 0, C % 32 == 0; R == 0 launches nothing. */
int ao_mxfp8_quantize_rowcol(const uint16_t* x, uint8_t* q_row, uint8_t* s_row,   /* e4m3 [R][C], e8m0 [R][C/32] */
                             uint8_t* q_col_t, uint8_t* s_col,                    /* e4m3 [C][R], e8m0 [R/32][C] */
                             int64_t R, int64_t C, int scaling_mode, void* stream);

/* The 3-D (per-expert) form: mxfp8_quantize_cuda_3d with (scale_block_dim1, scale_block_dim2) = (32, 1), logical scales
 * (torchao/prototype/moe_training/kernels/mxfp8/quant.py:1413-1440; csrc/cuda/mx_kernels/mxfp8_quantize.cuh:822-1290) --
 * every [R][C] matrix of the batch cast on its own, "column-major-per-expert" data.
 *   x bf16 [E][R][C] -> q_t e4m3fn [E][C][R], scale e8m0 [E][R/32][C]. */
int ao_mxfp8_quantize_colwise_3d(const uint16_t* x, uint8_t* q_t, uint8_t* scale_e8m0,
                                 int64_t E, int64_t R, int64_t C, int scaling_mode, void* stream);

/* Replaces aten::_scaled_grouped_mm as called from _compute_fwd_sm100
 * (torchao/prototype/moe_training/mxfp8_grouped_mm.py:541), with the numerics of
 * _emulated_mxfp8_scaled_grouped_mm_2d_3d (:959-1023):
 *   out[offs[e-1]:offs[e]] = dq(a_rows) @ dq(b[e])^T,  dq = fp8 * 2^(scale-127)
 *   a e4m3 [M_total][K]; a_scale e8m0 [M_total][K/32];
 *   b e4m3 [E][N][K] (each expert row-major [N][K]); b_scale e8m0 [E][N][K/32];
 *   offs int32 [E] cumulative group ends; out bf16 [M_total][N].  Rows past offs[E-1] are not written.
 * Scale layout is plain row-major (CDNA4 scaled-MFMA takes scales in VGPRs; the
 * cuBLAS 128x4 "blocked" swizzle is not read by any GEMM here; ao_mx_block_rearrange_2d_m_groups writes it as a data format). */
int ao_mxfp8_grouped_mm(const uint8_t* a, const uint8_t* a_scale,
                        const uint8_t* b, const uint8_t* b_scale,
                        const int32_t* offs, uint16_t* out, int64_t M_total,
                        int64_t N, int64_t K, int64_t E, void* stream);

/* _to_mxfp8_then_scaled_grouped_mm's forward in ONE launch (torchao/prototype/moe_training/mxfp8_grouped_mm.py:330-371, 552-594: to_mx(A, 32,
 * scaling_mode) followed by the grouped mm above; SURVEY.md 8 f1 for the MX format; native analogue of the cast: torchao/csrc/cuda/mx_kernels/
 * mxfp8_quantize.cuh:460-820).  a is the BF16 activation matrix [M_total][K]; the 1 x 32 cast runs inside the kernel's A-fill with the
 * arithmetic of ao_mxfp8_quantize_rowwise (same codes, same scales, so out is bit-identical to cast + ao_mxfp8_grouped_mm).
 * Decode-size groups only: ao_mxfp8_grouped_mm_dyn_fits(M_total, N, K, E) (host logic, no launch) is 1 when M_total <= 48 E, E <= 64,
 * K % 512 == 0, N % 16 == 0; other shapes return AO_ERR_INVALID_ARGUMENT -- cast and call ao_mxfp8_grouped_mm.  a and b_scale 16-byte aligned. */
int ao_mxfp8_grouped_mm_dyn_fits(int64_t M_total, int64_t N, int64_t K, int64_t E);
int ao_mxfp8_grouped_mm_dyn(const uint16_t* a, const uint8_t* b, const uint8_t* b_scale, const int32_t* offs, uint16_t* out,
                            int64_t M_total, int64_t N, int64_t K, int64_t E, int scaling_mode, void* stream);

/* Two expert-weight tensors of ONE shape [E][N][K] against the same activations in ONE launch: an MoE layer's w1 and w3 (the reference's
 * experts compute x @ w1 and x @ w3 by two calls of _to_mxfp8_then_scaled_grouped_mm, mxfp8_grouped_mm.py:56-239, casting x twice).
 * out1 / out3 bf16 [M_total][N] hold the values of two single calls: the same bits where the stream-K shares cut the tiles at the same k steps
 * (a cut tile's pieces are added in k order; another cut is another fp32 summation order -- single elements one bf16 ulp apart, the same from
 * launch to launch).  _dyn_pair: a is BF16, cast fused (as ao_mxfp8_grouped_mm_dyn);
 * _pair: a / a_scale are the caller's e4m3 codes / E8M0 scales.  Shapes: ao_mxfp8_grouped_mm_pair_fits (host logic; the _dyn conditions
 * with twice the tiles). */
int ao_mxfp8_grouped_mm_pair_fits(int64_t M_total, int64_t N, int64_t K, int64_t E);
int ao_mxfp8_grouped_mm_dyn_pair(const uint16_t* a, const uint8_t* b1, const uint8_t* b1_scale, const uint8_t* b3, const uint8_t* b3_scale,
                                 const int32_t* offs, uint16_t* out1, uint16_t* out3, int64_t M_total, int64_t N, int64_t K, int64_t E,
                                 int scaling_mode, void* stream);
int ao_mxfp8_grouped_mm_pair(const uint8_t* a, const uint8_t* a_scale, const uint8_t* b1, const uint8_t* b1_scale, const uint8_t* b3,
                             const uint8_t* b3_scale, const int32_t* offs, uint16_t* out1, uint16_t* out3, int64_t M_total, int64_t N,
                             int64_t K, int64_t E, void* stream);

/* The weight gradient of _to_mxfp8_then_scaled_grouped_mm: replaces the 2d-2d aten::_scaled_grouped_mm of _compute_wgrad
 * (torchao/prototype/moe_training/mxfp8_grouped_mm.py:712-796), with the numerics of _emulated_mxfp8_scaled_grouped_mm_2d_2d (:1026-1057):
 *   out[e][n][k] = bf16( sum_{m in [offs[e-1], offs[e])} dq(g)[m][n] dq(x)[m][k] ),  fp32 accumulation, one rounding.
 * The operands are byte for byte what ao_mxfp8_quantize_colwise writes for grad_out [M_total][N] and x [M_total][K] (no relayout, no 128 x 4
 * swizzle); the 32-token blocks lie on the global grid.  Any offsets: a block that straddles a group boundary lends its scale to both groups
 * and each sums its own tokens.  An empty group's [N][K] slab is zero, tokens past offs[E-1] contribute to nothing, M_total == 0 zeroes out.
 * M_total % 32 == 0, N % 16 == 0, K % 16 == 0, E < 65536, N M_total and K M_total below 2^31; the codes 16-byte aligned. */
int ao_mxfp8_grouped_mm_wgrad(const uint8_t* g_t, const uint8_t* g_scale,   /* e4m3 [N][M_total], e8m0 [M_total/32][N] */
                              const uint8_t* x_t, const uint8_t* x_scale,   /* e4m3 [K][M_total], e8m0 [M_total/32][K] */
                              const int32_t* offs, uint16_t* out,           /* int32 [E] cumulative ends; bf16 [E][N][K] */
                              int64_t M_total, int64_t N, int64_t K, int64_t E, void* stream);

/* The weight gradient of a dense MXFP8 linear (mx_mm.backward, torchao/prototype/moe_training/mxfp8_linear.py:208-255): the kernel above over
 * ONE group that holds every token, without an offs tensor -- out[n][k] = bf16( sum_m dq(g)[m][n] dq(x)[m][k] ), the bits of
 * ao_mxfp8_grouped_mm_wgrad with E = 1 and offs = [M].  The same operand layouts and checks; M == 0 zeroes out. */
int ao_mxfp8_mm_wgrad(const uint8_t* g_t, const uint8_t* g_scale,   /* e4m3 [N][M], e8m0 [M/32][N] */
                      const uint8_t* x_t, const uint8_t* x_scale,   /* e4m3 [K][M], e8m0 [M/32][K] */
                      uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream);   /* bf16 [N][K] */

/* Float8Tensor's aten::_grouped_mm with rowwise scales (float8_tensor.py:1085-1122 -> scaled_grouped_mm, RowWise recipes):
 *   out[offs[e-1]:offs[e]] = bf16( (a_rows @ b[e]^T)_f32 * scale_a[m] * scale_b[e][n] )
 *   a e4m3 [M_total][K]; scale_a fp32 [M_total]; b e4m3 [E][N][K]; scale_b fp32 [E][N]; offs int32 [E]; out bf16 [M_total][N].
 *   Rows past offs[E-1] are not written. */
int ao_fp8_grouped_mm(const uint8_t* a, const float* scale_a, const uint8_t* b, const float* scale_b,
                      const int32_t* offs, uint16_t* out, int64_t M_total, int64_t N, int64_t K,
                      int64_t E, void* stream);

/* ------------------------------------------------------------------------- *
 * MoE token-group padding (glue either side of the MXFP8 grouped GEMM)
 * ------------------------------------------------------------------------- */

/* Rows of the padded buffer: align_up(num_tokens + num_groups * alignment, alignment) -- the upper bound the
 * reference allocates so that no host sync is needed (quant.py:414-420).  Host-only helper. */
int64_t ao_moe_padded_rows(int64_t num_tokens, int64_t num_groups, int alignment);

/* Replaces torchao::fused_pad_token_groups (schema torchao/prototype/moe_training/kernels/mxfp8/quant.py:1244-1246;
 * semantics torch_pad_token_groups, quant.py:368-430).
 *   inputs  [num_tokens][dim] bf16 or fp32 (elem_bytes 2 or 4); offsets int32 [num_groups] cumulative group ends;
 *   padded  [ao_moe_padded_rows(...)][dim], every row written (groups copied to aligned starts, the rest zero);
 *   padded_starts / padded_ends int32 [num_groups]. */
int ao_moe_pad_token_groups(const void* inputs, const int32_t* offsets, void* padded,
                            int32_t* padded_starts, int32_t* padded_ends, int64_t num_tokens,
                            int64_t dim, int elem_bytes, int64_t num_groups, int alignment,
                            void* stream);

/* Replaces torchao::fused_unpad_token_groups (schema quant.py:1319-1321; semantics torch_unpad_token_groups,
 * quant.py:433-480): out[t] = padded[padded_starts[g] + t - offsets[g-1]] for the group g holding token t.
 * Tokens past offsets[num_groups-1] (the reference raises after a host sync) are written as zeros. */
int ao_moe_unpad_token_groups(const void* padded, const int32_t* offsets,
                              const int32_t* padded_starts, void* out, int64_t num_tokens,
                              int64_t dim, int elem_bytes, int64_t num_groups, void* stream);

/* Replaces torchao::mx_block_rearrange_2d_M_groups (schema torchao/prototype/moe_training/kernels/mxfp8/quant.py:969-973; host wrapper
 * csrc/cuda/mx_kernels/mxfp8_extension.cpp:178-300; semantics torch_to_blocked_2d_M_groups, quant.py:136-196, over to_blocked,
 * prototype/mx_formats/utils.py:31-72): E8M0 scales [rows][cols] whose rows are grouped by `offsets` (int32 [num_groups] cumulative
 * ends) -> the reference's "128 x 4 blocked" layout, every group padded to 128-row blocks:
 *   out [ao_mx_blocked_rows(rows, num_groups)][4 ceil(cols / 4)] bytes, every byte written (zero where no scale lands), 16-byte aligned;
 *   group g starts at out row sum_{h<g} 128 ceil(size_h / 128); tile (rb, cb) of a group at + (rb ncb + cb) 512 bytes, element (r, c)
 *   of a tile at (r % 32) 16 + (r / 32) 4 + c.
 * The GEMMs of this library take row-major scales; this is a data-format op for callers that hold the blocked layout.
 * ao_mx_blocked_rows = rows + 128 num_groups, the reference's no-host-sync upper bound (mxfp8_extension.cpp:221). */
int64_t ao_mx_blocked_rows(int64_t rows, int64_t num_groups);
int ao_mx_block_rearrange_2d_m_groups(const uint8_t* scales, const int32_t* offsets, uint8_t* out, int64_t rows, int64_t cols,
                                      int64_t num_groups, void* stream);
/* to_blocked of one matrix (prototype/mx_formats/utils.py:31-72): out [128 ceil(rows / 128)][4 ceil(cols / 4)] bytes, the same tiles. */
int ao_mx_to_blocked(const uint8_t* scales, uint8_t* out, int64_t rows, int64_t cols, void* stream);

/* ------------------------------------------------------------------------- *
 * One-shot all-reduce over peer-mapped buffers (TP row-parallel linears at decode sizes)
 * ------------------------------------------------------------------------- */

/* Peer-visible device memory for the flag blocks and staging buffers below, and its IPC handles.  The caching allocator's memory is
 * coarse-grained: a flag a REMOTE GPU writes may be served to the spinning owner from its local L2 for ever (two processes on ONE GPU
 * share that L2 and cannot show it).  kind 0 = hipDeviceMallocUncached (flag blocks), kind 1 = hipDeviceMallocFinegrained (staging);
 * zero-filled.  ao_peer_export writes ao_peer_handle_bytes() (64) opaque bytes any process of the node can ao_peer_import (maps the
 * peer's allocation, enabling peer access lazily); ao_peer_close unmaps an imported pointer, ao_peer_free releases an own one.  All
 * HOST-side, synchronous, not capturable. */
int ao_peer_alloc(void** ptr_out_host, int64_t bytes, int kind);
int ao_peer_free(void* ptr);
int ao_peer_handle_bytes(void);
int ao_peer_export(void* ptr, void* handle_out_host);
int ao_peer_import(const void* handle_host, void** ptr_out_host);
int ao_peer_close(void* imported_ptr);
/* How long a collective kernel waits for a peer before it gives up (1 ms .. 10 min, default 5000 ms; measured with the 100 MHz
 * constant clock on the device).  A launch that gives up sets bit 0 of its local_state[0] AND poisons its output (NaN / INT_MIN for the
 * all-reduce, zero rows for the all-to-all): a late rank never yields a plausible wrong result.  Process-wide. */
int ao_collective_set_timeout_ms(int ms);
int ao_collective_timeout_ms(void);

/* Bytes of the flag block every rank allocates (zero-filled) and maps into its peers, and of the rank-local state block (zero-filled,
 * never shared: a status word + one epoch counter per block).  Host-only helpers. */
int64_t ao_allreduce_flag_bytes(void);
int64_t ao_allreduce_state_bytes(void);

/* SUM (or, _op with op = 1, elementwise MAX) all-reduce of one small vector in ONE launch per rank ("direct / one-shot
 * algorithm for S <= ~1 MiB, never a ring on the fully connected 8-GPU xGMI mesh"; the caller-issued all-reduce of the reference's TP
 * harness, torchao/testing/utils.py:370-467; MAX is the row-amax exchange of the exact row-parallel protocol).  Every rank stages its
 * vector in device memory all peers have mapped (IPC), raises a flag in every peer's flag block, waits (bounded) for all flags, then
 * reads all `world` staged vectors and combines them in rank order (fp32 accumulation for bf16 / fp32, exact for int32):
 * bit-identical results on every rank.
 *   peer_data_host / peer_flags_host: HOST arrays of `world` DEVICE pointers, index = rank (own buffers at [rank]); every staging
 *     buffer is 2 x slot_bytes (double-buffered by epoch parity), every flag block ao_allreduce_flag_bytes() bytes, zero-filled once
 *     (ao_peer_alloc kinds 1 and 0);
 *   input / output: count elements of dtype (0 fp32, 1 bf16, 2 int32), count x size a multiple of 16 and <= slot_bytes; may alias;
 *   local_state: device uint32 [ao_allreduce_state_bytes() / 4]: word 0 is set to 1 if a peer did not arrive within the timeout
 *     (the output is then NaN / INT_MIN) -- check it wherever the host synchronises anyway; the rest are the per-block epoch counters
 *     the kernel bumps on every call (they live on the device so that a launch captured into a hipGraph replays correctly).  Every
 *     rank must make the same sequence of calls. */
int ao_allreduce_oneshot(void* const* peer_data_host, void* const* peer_flags_host, const void* input,
                         void* output, void* local_state, int64_t count, int dtype, int64_t slot_bytes,
                         int rank, int world, void* stream);
int ao_allreduce_oneshot_op(void* const* peer_data_host, void* const* peer_flags_host, const void* input,
                            void* output, void* local_state, int64_t count, int dtype, int op,
                            int64_t slot_bytes, int rank, int world, void* stream);

/* On-device all-to-all-v of MXFP8 token rows (expert-parallel dispatch without a host round trip for the split sizes).  Replaces the
 * Triton kernel torchao/prototype/moe_training/kernels/mxfp8/comms.py:318-460 (_mxfp8_all_to_all_v_kernel, _exchange_row_offsets) that
 * MXFP8OnDeviceAllToAllV.forward (:52-167) launches over symmetric memory.  Every rank has staged its e4m3 rows (ordered by destination
 * rank), its E8M0 scale rows and its int64 split vector (rows it sends to rank r) in buffers all peers have mapped; this rank pulls the
 * rows addressed to it: from rank q, rows [sum_{r < rank} splits_q[r], + splits_q[rank]) land at local rows [sum_{p < q} splits_p[rank], ..),
 * and out_splits[q] = splits_q[rank].  Barriers before (inputs staged everywhere) and after (staging may be overwritten) are inside
 * the launch; epochs live on the device (hipGraph-replayable); a peer that never arrives sets bit 0 of local_state[0] after the
 * collective timeout (nothing is read from it: out_splits of that peer = 0), more rows than max_out_rows sets bit 1 (the rows past the
 * end are not written), a peer's split prefix that reaches past its max_in_rows staged rows sets bit 2 (the read is clamped to them).
 *   peer_*_host: HOST arrays of `world` DEVICE pointers, index = rank (own buffers at [rank]); data / scale staging 16-byte aligned,
 *     flag blocks ao_moe_a2a_flag_bytes() bytes, zero-filled once; local_state: ao_moe_a2a_state_bytes() bytes, zero-filled once;
 *   row_bytes = D (e4m3), a multiple of 16; scale_row_bytes = D / 32.  Every rank must make the same sequence of calls. */
int64_t ao_moe_a2a_flag_bytes(void);
int64_t ao_moe_a2a_state_bytes(void);
int ao_moe_a2a_v(void* const* peer_data_host, void* const* peer_scales_host, void* const* peer_splits_host,
                 void* const* peer_flags_host, void* out_data, void* out_scales, int64_t* out_splits,
                 void* local_state, int64_t row_bytes, int64_t scale_row_bytes, int64_t max_in_rows,
                 int64_t max_out_rows, int rank, int world, void* stream);

/* ------------------------------------------------------------------------- *
 * fp8 activations x int4 weights (Float8DynamicActivationInt4WeightConfig)
 * ------------------------------------------------------------------------- */

/* Replaces mslk.f8i4bf16_rowwise as called by Int4Tensor's F.linear with activation_dtype = float8_e4m3fn
 * (torchao/quantization/quantize_/workflows/int4/int4_tensor.py:213-229; quant_api.py:630-699):
 *   xq e4m3 [M][K], x_scale fp32 [M] (per-row dynamic cast: ao_fp8_quantize_rowwise);
 *   qdata / scale_and_zero: the int4 weight in the tinygemm tile order with offset-8 codes (what Int4Tensor.tile_packed() builds from
 *   the PLAIN data; scale_and_zero bf16 [K/group_size][N][2], zero = 0 for the reference's symmetric flavour); bias bf16 [N] or NULL.
 *   y[m][n] = bf16( x_scale[m] * sum_g ( s[g][n] * sum_{k in g} xq[m][k] (q[n][k] - 8) + z[g][n] * sum_{k in g} xq[m][k] ) + bias[n] )
 * fp8 MFMA on the codes themselves, the scale applied per group to fp32 sums (no per-weight rounding).  N % 16 == 0, K % 128 == 0. */
int ao_fp8_int4_linear(const uint8_t* xq, const float* x_scale, const int32_t* qdata,
                       const uint16_t* scale_and_zero, const uint16_t* bias, uint16_t* y, int64_t M,
                       int64_t N, int64_t K, int group_size, void* stream);
/* The same linear on the bf16 activation, its per-row e4m3 cast (ao_fp8_quantize_rowwise's arithmetic: float8_tensor.py:167-253 as
 * Int4Tensor's F.linear applies it, int4_tensor.py:205-212) fused into the launch -- SURVEY.md 8 f1 for this path.  Shapes:
 * ao_fp8_int4_dynamic_fits (M <= 16, M * (K + 16) <= 65536).  Same bits as cast + ao_fp8_int4_linear. */
int ao_fp8_int4_dynamic_fits(int64_t M, int64_t N, int64_t K);
int ao_fp8_int4_dynamic_linear(const uint16_t* x, const int32_t* qdata, const uint16_t* scale_and_zero,
                               const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                               int group_size, void* stream);

/* ------------------------------------------------------------------------- *
 * Expert-parallel token regrouping (between the all-to-all and the grouped GEMM)
 * ------------------------------------------------------------------------- */

/* Replaces generate_permute_indices (torchao/prototype/moe_training/ep/kernels.py:132-214; Triton `_fill_indices_kernel` :13-60,
 * semantics of fill_indices_cpu :94-129).
 *   tokens_per_expert_group int32 [num_ranks * experts_per_rank], rank-major counts of the tokens this rank received;
 *   start_workspace         int32 [num_ranks * experts_per_rank] scratch (exclusive prefix sum of the counts);
 *   permuted_indices        int32 [max_len]: source row of every expert-major position, -1 for alignment padding and the tail;
 *   m_sizes / m_offsets     int32 [experts_per_rank]: align_up(max(tokens of expert, alignment), alignment) and its inclusive cumsum. */
int ao_moe_permute_indices(const int32_t* tokens_per_expert_group, int32_t* start_workspace,
                           int32_t* permuted_indices, int32_t* m_sizes, int32_t* m_offsets,
                           int64_t experts_per_rank, int64_t num_ranks, int64_t max_len,
                           int alignment, void* stream);

/* Replaces the row gather `vstack(x, 0)[permuted_indices]` of permute_and_pad / _PermuteMXFP8FwdHPBwd.forward (ep/permute.py:86-96,
 * 195-198) and of _UnpermuteHPFwdMXFP8Bwd.backward (ep/unpermute.py:57-98): out[i] = inputs[indices[i]] when 0 <= indices[i] <
 * num_rows_in, else zeros (index -1 and index num_rows_in are the reference's appended zero row).  Rows are row_bytes bytes of any
 * dtype (bf16 tokens, e4m3 data, e8m0 scales). */
int ao_moe_gather_rows(const void* inputs, const int32_t* indices, void* out, int64_t num_rows_in,
                       int64_t num_rows_out, int64_t row_bytes, void* stream);

/* Replaces the row scatter `out[permuted_indices] = y; out[:-1]` of _UnpermuteHPFwdMXFP8Bwd.forward / _unpermute_bf16
 * (ep/unpermute.py:36-41, 152-158): out[indices[i]] = inputs[i] when 0 <= indices[i] < num_rows_out (rows sent to the dummy row are
 * dropped; rows of `out` no index names are left untouched, as in the reference's new_empty). */
int ao_moe_scatter_rows(const void* inputs, const int32_t* indices, void* out, int64_t num_rows_in,
                        int64_t num_rows_out, int64_t row_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Dynamic-activation linears with the activation cast fused in (decode sizes)
 * ------------------------------------------------------------------------- */

/* 1 when the fused entry points below accept the shape: 0 < M <= 16, M * (K + 16) <= 65536 (the cast activation lives in
 * LDS), N % 16 == 0, K % 128 == 0.  Host-only helper. */
int ao_dyn_linear_fits(int64_t M, int64_t N, int64_t K);

/* Replaces the Int8Tensor F.linear with dynamic activation quantisation as ONE launch: Int8Tensor.from_hp(x, PerRow)
 * (int8_tensor.py:176-248) followed by _int_scaled_matmul + weight scale (int8/kernels.py:114-144, int8_tensor.py:305-359).
 * Same bits as ao_int8_quantize_rowwise + ao_int8_scaled_mm.
 *   x bf16 [M][K]; wq int8 [N][K]; w_scale fp32 [N]; bias bf16 [N] or NULL; y bf16 [M][N]. */
int ao_int8_dynamic_linear(const uint16_t* x, const int8_t* wq, const float* w_scale,
                           const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                           void* stream);

/* Same for float8 rowwise: Float8Tensor.from_hp(x, PerRow) (float8_tensor.py:167-253) + aten::_scaled_mm with rowwise scales
 * (float8/inference.py:104-123).  Same bits as ao_fp8_quantize_rowwise + ao_fp8_scaled_mm at these sizes.
 *   x bf16 [M][K]; wq e4m3fn [N][K]; w_scale fp32 [N]; bias bf16 [N] or NULL; y bf16 [M][N]. */
int ao_fp8_dynamic_linear(const uint16_t* x, const uint8_t* wq, const float* w_scale,
                          const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, int64_t K,
                          void* stream);

/* ---- K-sharded (row-parallel) 8-bit linears: the unsharded result from sharded operands ---------------------------------
 * torchao delegates TP to its caller (DTensor / vLLM slice the subclasses: int8_tensor.py:362-422, float8_tensor.py:732-839;
 * harness torchao/testing/utils.py:370-519).  A caller that wants the UNSHARDED linear's bits from K shards needs the
 * activation scale over the full K and the scale epilogue applied once, after the partial sums are added:
 *   amax_local = ao_rowwise_amax(x_shard);  all_reduce(MAX, amax);  q_shard = ao_*_quantize_rowwise_amax(x_shard, amax);
 *   acc = ao_int8_int_mm / ao_fp8_mm_f32 (q_shard, w_shard);  all_reduce(SUM, acc);  y = ao_*_scale_epilogue(acc).
 * `ldx` is the row stride of x in elements (a column slice of the full activation needs no copy). */
int ao_rowwise_amax(const uint16_t* x, int64_t ldx, float* amax, int64_t M, int64_t K, void* stream);
/* Int8Tensor.from_hp arithmetic (int8_tensor.py:191-230) with the row's amax given instead of reduced over x's K columns. */
int ao_int8_quantize_rowwise_amax(const uint16_t* x, int64_t ldx, const float* amax, int8_t* q,
                                  float* scale, int64_t M, int64_t K, void* stream);
/* Float8Tensor.from_hp arithmetic (float8_tensor.py:167-253) with the row's amax given. */
int ao_fp8_quantize_rowwise_amax(const uint16_t* x, int64_t ldx, const float* amax, uint8_t* q,
                                 float* scale, int64_t M, int64_t K, void* stream);
/* c fp32 [M][N] = a e4m3fn [M][K] @ b e4m3fn [N][K]^T, no scales: the accumulator of aten::_scaled_mm
 * (float8/inference.py:104-123) before its scale epilogue. */
int ao_fp8_mm_f32(const uint8_t* a, const uint8_t* b, float* c, int64_t M, int64_t N, int64_t K,
                  void* stream);
/* y = bf16( bf16(f32(acc) * x_scale[m]) * w_scale[n] (+ bias[n]) ): the epilogue of int8_tensor.py:315-359 on its own. */
int ao_int8_scale_epilogue(const int32_t* acc, const float* x_scale, const float* w_scale,
                           const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, void* stream);
/* y = bf16( acc * scale_a[m] * scale_b[n] (+ bias[n]) ): the epilogue of aten::_scaled_mm (rowwise) on its own. */
int ao_fp8_scale_epilogue(const float* acc, const float* scale_a, const float* scale_b,
                          const uint16_t* bias, uint16_t* y, int64_t M, int64_t N, void* stream);

/* ---- MX dense linears: MXFP4 (e2m1) / MXFP8 (e4m3) elements, E8M0 scales over 1 x 32 blocks along K -------------------------
 * The GEMM of torchao's MXTensor linear (torchao/prototype/mx_formats/mx_tensor.py:760-880, _addmm_mx_dispatch; the weight of
 * MXDynamicActivationMXWeightConfig, inference_workflow.py:80-171).  fmt is the scaled MFMA's format code: AO_MX_FMT_E4M3 (0) or
 * AO_MX_FMT_E2M1 (4).  Codes are row-major and K-contiguous: e4m3 [rows][K], e2m1 packed [rows][K/2] (element 2i in the low nibble,
 * pack_uint4, kernels.py:155-160); scales E8M0 bytes [rows][K/32] in plain row-major layout (to_mx(..., is_swizzled_scales=False); no
 * 128 x 4 swizzle).  Shapes: M >= 0, N >= 1, K a positive multiple of 32, each operand < 2 GiB; ragged edges are masked.  DESIGN.md 4.10. */
#define AO_MX_FMT_E4M3 0
#define AO_MX_FMT_E2M1 4
/* Replaces to_mx(x, torch.float4_e2m1fn_x2, 32, mode) (mx_tensor.py:228-409; RCEIL :161-224; e2m1 rounding
 * custom_fp_utils._f32_to_floatx_unpacked): x bf16 [R][C], C % 32 == 0 -> q [R][C/2] packed codes, scale_e8m0 [R][C/32];
 * byte for byte the reference's.  x and q 16-byte aligned. */
int ao_mxfp4_quantize_rowwise(const uint16_t* x, uint8_t* q, uint8_t* scale_e8m0, int64_t R, int64_t C, int scaling_mode, void* stream);
/* out bf16 [M][N] = bf16( sum_k dq(a)[m][k] dq(b)[n][k] + bias[n] ), dq = element * 2^(scale - 127), fp32 accumulation, one rounding
 * (the numerics of the reference's EMULATED path, mx_tensor.py:828-841, without its bf16 rounding of the dequantised operands).  a / a_scale:
 * the activation's codes; b / b_scale: the weight as stored [N][...]; bias bf16 [N] or NULL.  a and b 16-byte aligned. */
int ao_mx_linear(int fmt, const uint8_t* a, const uint8_t* a_scale, const uint8_t* b, const uint8_t* b_scale, const uint16_t* bias,
                 uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream);
/* to_mx(x, elem, 32, scaling_mode) followed by ao_mx_linear in ONE launch, for the shapes the streaming form takes
 * (ao_mx_dynamic_linear_fits, host logic: 1 when the route is mx_linear_stream_kernel); bit-identical to the cast + ao_mx_linear.
 * Other shapes return AO_ERR_INVALID_ARGUMENT.  x bf16 [M][K], 16-byte aligned. */
int ao_mx_dynamic_linear_fits(int fmt, int64_t M, int64_t N, int64_t K);
int ao_mx_dynamic_linear(int fmt, const uint16_t* x, const uint8_t* b, const uint8_t* b_scale, const uint16_t* bias, uint16_t* out,
                         int64_t M, int64_t N, int64_t K, int scaling_mode, void* stream);
/* The route both MX linear entries launch (host logic only): out[cap >= 7] = kernel (0 = invalid shape, 1 mx_linear_stream_kernel,
 * 2 mx_linear_tile_kernel), waves per workgroup, m-tiles of 16 per workgroup, tile rows, tile columns, grid x, grid y.  The streaming
 * form up to 64 rows (e4m3) / 32 rows (e2m1), the 128 x 128 LDS-tiled form beyond. */
int ao_mx_linear_route(int fmt, int64_t M, int64_t N, int64_t K, int32_t* out, int cap);
/* "mx_linear_stream_kernel", "mx_linear_tile_kernel" or "invalid": the kernel of that route. */
const char* ao_mx_linear_kernel_name(int fmt, int64_t M, int64_t N, int64_t K);
/* Measurement only: force the form of the calling thread's MX linears (0 the product route, 1 streaming, 2 tiled); the route queries
 * report the forced form. */
int ao_mx_linear_set_form(int form);

/* ---- int8 / float8 WEIGHT-ONLY linears: bf16 activation x 8-bit weight (wo8_kernels.hip) ----------------------------------------------
 * Replaces the weight-only branch of Int8Tensor's F.linear (quantize_/workflows/int8/int8_tensor.py:346-359, what Int8WeightOnlyConfig,
 * quant_api.py:702-770, produces) and of Float8Tensor's (quantize_/workflows/float8/float8_tensor.py:460-469 with dequantize :255-275,
 * Float8WeightOnlyConfig, quant_api.py:1031-1100).  x bf16 [M, K]; wq int8 or float8_e4m3fn [N, K], K-contiguous; w_scale fp32, one per
 * row (scale_count = N) or one for the tensor (scale_count = 1); bias bf16 [N] or null; out bf16 [M, N].  fp32 accumulation, every
 * bf16(.) round-to-nearest-even:
 *   int8: t = bf16(sum_k x q);  u = bf16(f32(t) f32(bf16(s[n])));  y = bf16(f32(u) + bias[n])
 *   e4m3: w = bf16(f32(q) s[n]) per element;  t = bf16(sum_k x w);  y = bf16(f32(t) + bias[n])
 * M >= 0 (M = 0: OK, nothing launched), N >= 1, K a positive multiple of 16 up to 2^31 - 1024, M K and N K below 2^31.  x and wq 16-byte aligned; w_scale
 * 4-byte, bias and out 2-byte aligned. */
#define AO_WO8_FMT_INT8 0
#define AO_WO8_FMT_E4M3 1
int ao_wo8_linear(int fmt, const uint16_t* x, const void* wq, const float* w_scale, int64_t scale_count, const uint16_t* bias,
                  uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream);
/* The route ao_wo8_linear launches (host logic only; the dispatch of int8_tensor.py:336-359 / float8_tensor.py:460-469 has one path, this
 * library two forms): out[cap >= 7] = kernel (0 = no kernel takes the shape, 1 wo8_stream_kernel, 2 wo8_tile_kernel), waves per
 * workgroup, m-tiles of 16 per workgroup, tile rows, tile columns, grid x, grid y. */
int ao_wo8_linear_route(int fmt, int64_t M, int64_t N, int64_t K, int32_t* out, int cap);
/* Measurement only (no reference counterpart: int8_tensor.py:346-359 / float8_tensor.py:460-469 have one path): force the form of the
 * calling thread's weight-only linears (0 the product route, 1 streaming, 2 tiled); the route query reports the forced form. */
int ao_wo8_linear_set_form(int form);

/* ---- blockwise float8 linears: 1 x 128 activation blocks, 128 x 128 weight blocks, fp32 scales (fp8_block_kernels.hip) ----------------
 * Float8DynamicActivationFloat8WeightConfig with granularity [PerBlock([1, 128]), PerBlock([128, 128])] (quant_api.py:1112-1297), the layout
 * of the DeepSeek-V3 / Qwen3 FP8 checkpoints (weight_scale_inv = the [N/128][K/128] scale).  Upstream runs it on SM 8.9 / XPU only
 * (torchao/float8/inference.py:306-310) through a Triton GEMM (quantize_/workflows/float8/kernels.py:56-128).  Codes are e4m3fn bytes,
 * row-major and K-contiguous.  Shapes of the linears: M >= 0 (M = 0: OK, nothing launched), N >= 1 (ragged N and M are masked; b_scale has
 * ceil(N / 128) rows), K a positive multiple of 128, each operand below 2 GiB.  x / q / a / b 16-byte aligned, scales 4-byte, bias and out
 * 2-byte.  Null pointers and bad shapes are rejected on the host before any launch.  DESIGN.md 4.12. */
/* The stream form runs up to this many rows, the 128 x 128 LDS-tiled form beyond: the hand-over with the least time summed over the
 * Llama-3-8B five shapes and M = 16 .. 256 with each form forced (profiles/fp8_block_linear.jsonl). */
#define AO_FP8_BLOCK_STREAM_MAX_ROWS 192
/* Replaces Float8Tensor.from_hp(x, e4m3fn, PerBlock([1, 128])), kernel_choice "torch" (float8_tensor.py:233-242, quant_primitives.py:2173-2212,
 * :2271-2287): x bf16 [M][K] -> q [M][K], scale fp32 [M][K/128] = f32(bf16(amax_block / 448)), q = e4m3_sat(f32(x) / scale); byte for byte
 * the reference's (a block of zeros: scale 0, NaN codes).  No row-wide amax pass. */
int ao_fp8_quantize_block_1x128(const uint16_t* x, uint8_t* q, float* scale, int64_t M, int64_t K, void* stream);
/* The same cast with PerBlock([128, 128]) (same lines): w bf16 [N][K], N and K multiples of 128 -> q [N][K], scale fp32 [N/128][K/128]. */
int ao_fp8_quantize_block_128x128(const uint16_t* w, uint8_t* q, float* scale, int64_t N, int64_t K, void* stream);
/* Replaces blockwise_fp8_gemm (kernels.py:56-128, :85-97 the loop; float8_tensor.py:433-447 the call and the bias).  Per output element, fp32:
 *   acc = 0;  for kb ascending: p = sum of the block's 128 products a[m][k] b[n][k];  acc += (p * a_scale[m][kb]) * b_scale[n / 128][kb]
 *   t = bf16(acc);  out = bias ? bf16(f32(t) + f32(bias[n])) : t      (bf16 before the bias; bf16 out whatever the bias)
 * K parts are cut at multiples of 128 and added in part order: a launch is reproducible.  a [M][K], a_scale [M][K/128], b [N][K],
 * b_scale [ceil(N/128)][K/128], bias bf16 [N] or NULL, out bf16 [M][N]. */
int ao_fp8_block_linear(const uint8_t* a, const float* a_scale, const uint8_t* b, const float* b_scale, const uint16_t* bias, uint16_t* out,
                        int64_t M, int64_t N, int64_t K, void* stream);
/* ao_fp8_quantize_block_1x128 followed by ao_fp8_block_linear in ONE launch (float8_tensor.py:433-447 does the two steps), for the shapes the
 * streaming form takes (ao_fp8_block_dynamic_linear_fits, host logic: 1 when the route is fp8_block_stream_kernel); bit-identical to the
 * two launches.  Other shapes return AO_ERR_INVALID_ARGUMENT.  x bf16 [M][K], 16-byte aligned. */
int ao_fp8_block_dynamic_linear_fits(int64_t M, int64_t N, int64_t K);
int ao_fp8_block_dynamic_linear(const uint16_t* x, const uint8_t* b, const float* b_scale, const uint16_t* bias, uint16_t* out, int64_t M,
                                int64_t N, int64_t K, void* stream);
/* The route both blockwise linear entries launch (host logic only; kernels.py:56-128 has one kernel, this library two forms):
 * out[cap >= 7] = kernel (0 = invalid shape or more than 65535 grid rows, 1 fp8_block_stream_kernel, 2 fp8_block_tile_kernel), waves per
 * workgroup, m-tiles of 16 per workgroup, tile rows, tile columns, grid x, grid y. */
int ao_fp8_block_linear_route(int64_t M, int64_t N, int64_t K, int32_t* out, int cap);
/* "fp8_block_stream_kernel", "fp8_block_tile_kernel" or "invalid": the kernel of that route (kernels.py:56-128). */
const char* ao_fp8_block_linear_kernel_name(int64_t M, int64_t N, int64_t K);
/* Measurement only (no reference counterpart: kernels.py:56-128 has one path): force the form of the calling thread's blockwise linears
 * (0 the product route, 1 streaming, 2 tiled); the route queries report the forced form. */
int ao_fp8_block_linear_set_form(int form);

/* ---- blockwise float8 grouped GEMM for MoE experts (fp8_block_kernels.hip) -----------------------------------------------
 * The routed experts of the DeepSeek-V3 / Qwen3 FP8 checkpoints: token group e = rows [offs[e-1], offs[e]) of a (offs[-1] = 0) against
 * expert e, the chain of ao_fp8_block_linear per output element, in fp32, no bias:
 *   acc = 0;  for kb ascending: p = sum of the block's 128 products a[m][k] b[e][n][k];  acc += (p * a_scale[m][kb]) * b_scale[e][n / 128][kb]
 *   out[m][n] = bf16(acc)
 * Upstream has the operation as a training prototype only (torchao/prototype/moe_training/blockwise_fp8/grouped_mm.py with
 * grouped_mm_backend.py: DeepGEMM, or an emulation that dequantizes both operands to bf16, blockwise_fp8_training/grouped_kernels.py:78-93;
 * its training side here: "blockwise float8 TRAINING of the MoE grouped GEMM" below);
 * Float8Tensor's aten._grouped_mm refuses block scales (float8_tensor.py:1085-1122).
 * a e4m3fn [M_total][K]; a_scale fp32 [M_total][K/128]; b e4m3fn [E][N][K], every expert row-major and K-contiguous as the checkpoint
 * stores it; b_scale fp32 [E][ceil(N/128)][K/128] (weight_scale_inv, stacked); offs int32 [E], cumulative group ends, read on the device
 * (no host sync); out bf16 [M_total][N].  Rows past offs[E-1] are not written.  Empty groups are legal anywhere; group sizes need no
 * alignment.  A group's row range is clamped to [0, M_total] and a non-increasing pair of offs is an empty group, so a bad offs cannot
 * address outside a or out.  K parts are cut at multiples of 128 and added in part order: a launch is reproducible.
 * M_total >= 0 (0: OK, nothing launched), N >= 1 (ragged N masked), K a positive multiple of 128, 1 <= E <= 65535; M_total K and the
 * per-expert N K below 2^31 (the expert base is 64-bit: the whole b may pass 2 GiB).  a and b 16-byte aligned, the scales and offs 4-byte,
 * out 2-byte.  Null pointers and bad shapes are rejected on the host before any launch. */
/* The route keys on the mean group size ceil(M_total / E), all the host knows without a sync: fp8_block_grouped_stream_kernel up to this
 * many rows, fp8_block_grouped_tile_kernel beyond.  It started at the dense family's 192; the sweep of tools/bench_fp8_block_grouped.py
 * --sweep (each form forced over uniform groups of 16 .. 512 rows on one EP-8 rank's DeepSeek-V3 and Qwen3-235B experts,
 * profiles/fp8_block_grouped.jsonl) moved it: summed over the four shapes and eleven group sizes the hand-over at 16 rows costs
 * 10126 us, at 0 rows 10173, at 32 rows 10275, at 192 rows 19270.  A group of up to 128 rows is ONE tile of the tiled form whatever its
 * size, while the stream form walks it 16 rows at a time. */
#define AO_FP8_BLOCK_GROUPED_STREAM_MAX_ROWS 16
int ao_fp8_block_grouped_mm(const uint8_t* a, const float* a_scale, const uint8_t* b, const float* b_scale, const int32_t* offs, uint16_t* out,
                            int64_t M_total, int64_t N, int64_t K, int64_t E, void* stream);
/* The route of that launch (host logic only; grouped_kernels.py:78-93 has one path, this library two forms): out[cap >= 7] = kernel (0 =
 * invalid shape or more than 65535 grid rows, 1 fp8_block_grouped_stream_kernel, 2 fp8_block_grouped_tile_kernel), waves per workgroup,
 * m-tiles of 16 per pass or workgroup, tile rows, tile columns, grid x, grid y (stream: E; tile: ceil(M_total / 128) + E, the host's upper
 * bound on the tile count). */
int ao_fp8_block_grouped_mm_route(int64_t M_total, int64_t N, int64_t K, int64_t E, int32_t* out, int cap);
/* "fp8_block_grouped_stream_kernel", "fp8_block_grouped_tile_kernel" or "invalid": the kernel of that route. */
const char* ao_fp8_block_grouped_mm_kernel_name(int64_t M_total, int64_t N, int64_t K, int64_t E);
/* Measurement only (no reference counterpart): force the form of the calling thread's blockwise grouped GEMMs (0 the product route,
 * 1 streaming, 2 tiled); the route queries report the forced form. */
int ao_fp8_block_grouped_mm_set_form(int form);

/* ---- blockwise float8 TRAINING: the block-local casts and the weight-gradient GEMM (fp8_block_train_kernels.hip) --------
 * fp8_blockwise_mm of torchao/prototype/blockwise_fp8_training/linear.py:98-211.  The contract of the casts is the reference's torch
 * functions (kernels.py:1031-1156: torch_blockwise_scale_act_quant_lhs, _act_quant_rhs, _weight_quant):
 *   scale = f32(448 / max(f64(amax_block), 1e-12));  q = e4m3fn(clamp(f32(x) * scale, -448, 448));  the outputs hold inv = 1 / scale,
 * the RECIPROCAL scales the GEMMs multiply by.  This is the float8 training cast's arithmetic (ao_fp8_train_cast), not that of the
 * inference block casts above (ao_fp8_quantize_block_1x128: scale = bf16(amax / 448), q = x / scale): a block of zeros gives scale
 * f32(448 / 1e-12) and codes 0 here, scale 0 and NaN codes there.  The 128 x 1 direction clamps the amax at bf16(1e-12) = 1.00186e-12
 * before it widens it, as kernels.py:1096 does (only the reciprocal of a block with a smaller amax shows it; its codes are 0 either way).
 * One launch each, one read of the input, no amax pre-pass, no allocation, no synchronisation, no atomics.
 *
 * ao_fp8_block_train_cast: x bf16 [R][C], either or both directions; a null (codes, scales) pair skips that direction:
 *   rows   : 1 x 128 blocks along the last dimension, q_row [R][C], inv_row [R][C/128] row-major (ao_fp8_block_linear's a_scale); R >= 1
 *   columns: 128 x 1 blocks along dim 0, stored transposed, q_col_t [C][R], inv_col [R/128][C] -- the bytes of both
 *            act_quant_transposed_lhs (grad_output) and act_quant_rhs (x); R % 128 == 0
 * C % 128 == 0.  An empty matrix returns OK without a launch; other shapes are refused before any launch.
 * ao_fp8_block_train_cast_weight: w bf16 [N][K], 128 x 128 blocks, N and K multiples of 128; either or both layouts:
 *   q [N][K] with inv [N/128][K/128];  q_t [K][N] with inv_t [K/128][N/128] (the transposes: a block's codes do not depend on the layout).
 * x / w and the codes 16-byte aligned, the scales 4-byte. */
int ao_fp8_block_train_cast(const uint16_t* x, uint8_t* q_row, float* inv_row, uint8_t* q_col_t, float* inv_col, int64_t R, int64_t C,
                            void* stream);
int ao_fp8_block_train_cast_weight(const uint16_t* w, uint8_t* q, float* inv, uint8_t* q_t, float* inv_t, int64_t N, int64_t K, void* stream);
/* The weight gradient grad_output^T @ x on the column casts (kernels.py:320-379, triton_fp8_gemm_1x128_128x1).  Per output element, fp32:
 *   acc = 0;  for token block mb ascending: p = sum over the block's 128 tokens of g_t[n][m] x_t[k][m] (one scaled MFMA onto a zero
 *   accumulator);  acc += (p * g_inv[mb][n]) * x_inv[mb][k];  out[n][k] = bf16(acc).
 * No split along the tokens: a launch is reproducible.  M, N and K multiples of 128 (N, K > 0), each operand below 2^31 bytes; M == 0
 * writes zeros.  The codes and g_inv 16-byte aligned, x_inv 4-byte, out 2-byte.  Violations are refused on the host before any launch. */
int ao_fp8_block_mm_wgrad(const uint8_t* g_t, const float* g_inv,   /* e4m3 [N][M], fp32 [M/128][N] */
                          const uint8_t* x_t, const float* x_inv,   /* e4m3 [K][M], fp32 [M/128][K] */
                          uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream);  /* bf16 [N][K] */

/* ---- blockwise float8 TRAINING of the MoE grouped GEMM (fp8_block_train_kernels.hip) ------------------------------------
 * _Float8BlockwiseGroupedMM of torchao/prototype/moe_training/blockwise_fp8/grouped_mm.py:98-265.  The forward and grad_A are
 * ao_fp8_block_grouped_mm on the casts above (rows of A / grad_output, the 3-D weight cast below); the two entries here are what was
 * missing.
 *
 * ao_fp8_block_train_cast_weight_3d: ao_fp8_block_train_cast_weight over a stack of experts, w bf16 [E][N][K], in one launch and one
 * read of w: expert e's outputs are byte for byte those of the 2-D entry on w[e], at e N K (codes) and e (N/128)(K/128) (scales) of
 *   q [E][N][K] with inv [E][N/128][K/128]  (the forward's B of ao_fp8_block_grouped_mm);
 *   q_t [E][K][N] with inv_t [E][K/128][N/128]  (grad_A's B).  A null pair skips that layout.
 * N and K multiples of 128, 1 <= E <= 65535, at most 65535 row tiles (E N / 128); an empty tensor returns OK without a launch.  No
 * allocation, no synchronisation, no atomics; every index is 64-bit.  w and the codes 16-byte aligned, the scales 4-byte. */
int ao_fp8_block_train_cast_weight_3d(const uint16_t* w, uint8_t* q, float* inv, uint8_t* q_t, float* inv_t, int64_t E, int64_t N, int64_t K,
                                      void* stream);
/* The grouped weight gradient: ao_fp8_block_mm_wgrad per token group, on the column casts of the WHOLE token matrix (their 128-token blocks
 * sit on the global grid, whatever offs is -- what the reference's emulated wgrad feeds torch._grouped_mm, grouped_mm_backend.py:158-194).
 * Group e = tokens [lo, hi) = offs[e-1], offs[e] clamped to [0, M] (offs[-1] = 0); a non-increasing pair is an empty group.  Per output
 * element (e, n, k), fp32:
 *   acc = 0;  for every token block mb that meets [lo, hi), ascending: p = sum over the block's tokens INSIDE [lo, hi) of
 *   g_t[n][m] x_t[k][m] (one scaled MFMA with unit scales onto a zero accumulator, the foreign tokens' codes zeroed in registers);
 *   acc += (p * g_inv[mb][n]) * x_inv[mb][k];  out[e][n][k] = bf16(acc).
 * An empty group stores zeros; tokens at or past offs[E-1] contribute to nothing; group ends need no alignment.  No split along the
 * tokens: a launch is reproducible.  offs is read on the device; NULL means one group of every token (E must be 1).
 * M, N and K multiples of 128 (N, K > 0), 1 <= E <= 65535, N M and K M below 2^31; M == 0 writes zeros.  The codes and g_inv 16-byte
 * aligned, x_inv and offs 4-byte, out 2-byte.  Null pointers other than offs and bad shapes are refused on the host before any launch. */
int ao_fp8_block_grouped_mm_wgrad(const uint8_t* g_t, const float* g_inv,   /* e4m3 [N][M], fp32 [M/128][N] */
                                  const uint8_t* x_t, const float* x_inv,   /* e4m3 [K][M], fp32 [M/128][K] */
                                  const int32_t* offs,                      /* int32 [E] cumulative ends, device; NULL = one group of every token */
                                  uint16_t* out,                            /* bf16 [E][N][K] */
                                  int64_t M, int64_t N, int64_t K, int64_t E, void* stream);

/* ---- NVFP4 linears: e2m1 codes, one e4m3 scale per 1 x 16 block, an optional fp32 per-tensor scale (nvfp4_kernels.hip) -----------------
 * NVFP4Tensor of prototype/mx_formats/nvfp4_tensor.py and the two configs of inference_workflow.py:173-400.  Codes are packed two a byte
 * along K, element 2i in the low nibble of byte i; block scales are float8_e4m3fn bytes, ROW-MAJOR [rows][K/16] (no 128 x 4 swizzle);
 * per-tensor scales are read through device pointers, NULL meaning none.  The arithmetic contracts are those of csrc/quant_math.h
 * ("NVFP4"); DESIGN.md 4.14.  Null pointers and bad shapes are rejected on the host before any launch. */
#define AO_NVFP4_KIND_WEIGHT_ONLY 0
#define AO_NVFP4_KIND_DYNAMIC 1
/* Replaces per_tensor_amax_to_scale(torch.max(torch.abs(x))) (nvfp4_tensor.py:605-607, :756-769): x bf16 [R][C], C a multiple of 16 ->
 * out[0] = max|x| / 2688 in fp32, NaN if x holds one.  Three launches on the stream, no host read; x 16-byte, out 4-byte aligned. */
int ao_nvfp4_amax_scale(const uint16_t* x, float* out, int64_t R, int64_t C, void* stream);
/* Replaces nvfp4_quantize (nvfp4_tensor.py:772-854), the reference's bytes: x bf16 [R][C] contiguous, C a multiple of 16 -> q [R][C/2],
 * scale_e4m3 [R][C/16]; per_tensor_scale a device pointer to one fp32 or NULL.  x 16-byte, q 8-byte aligned. */
int ao_nvfp4_quantize(const uint16_t* x, const float* per_tensor_scale, uint8_t* q, uint8_t* scale_e4m3, int64_t R, int64_t C, void* stream);
/* Replaces the weight-only branch of nvfp4_linear (nvfp4_tensor.py:593-596: F.linear(x, weight.dequantize(bf16), bias), dequantize
 * :199-257): w = bf16(f32(code) (p f32(s8))) per element; out = bf16(sum_k x w + bias), fp32 accumulation, one rounding.  x bf16 [M][K],
 * wq [N][K/2], w_scale [N][K/16], bias bf16 [N] or NULL, out bf16 [M][N].  M >= 0 (M = 0: OK, nothing launched), N >= 1, K a positive
 * multiple of 16 up to 2^31 - 1024, M K and N K below 2^31.  x 16-byte aligned; the codes 16-byte and the block scales 2-byte aligned
 * (8-byte and 1-byte where K is not a multiple of 32); the per-tensor scale 4-byte, bias and out 2-byte. */
int ao_nvfp4_wo_linear(const uint16_t* x, const uint8_t* wq, const uint8_t* w_scale, const float* w_per_tensor_scale, const uint16_t* bias,
                       uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream);
/* Replaces _addmm_nvfp4_dispatch (nvfp4_tensor.py:487-578: torch._scaled_mm on sm100, then the per-tensor scales and the bias):
 * acc = sum_k (a_code a_s8)(b_code b_s8) in fp32.  Neither per-tensor scale: out = bf16(acc + bias).  Otherwise t = bf16(acc);
 * u = bf16(f32(t) f32(bf16(P))), P = pa pb (fp32) or the one present;  out = bias ? bf16(f32(u) + f32(bias)) : u.  a [M][K/2],
 * a_scale [M][K/16], b [N][K/2] (the weight as stored), b_scale [N][K/16].  Shapes and alignment as ao_nvfp4_wo_linear. */
int ao_nvfp4_linear(const uint8_t* a, const uint8_t* a_scale, const float* a_per_tensor_scale, const uint8_t* b, const uint8_t* b_scale,
                    const float* b_per_tensor_scale, const uint16_t* bias, uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream);
/* The route ao_nvfp4_wo_linear (kind 0) / ao_nvfp4_linear (kind 1) launch (host logic only; nvfp4_tensor.py:581-619 has one path per
 * kind, this library two forms): out[cap >= 7] = kernel (0 = no kernel takes the shape, 1 nvfp4_stream_kernel, 2 nvfp4_tile_kernel),
 * waves per workgroup, m-tiles of 16 per workgroup, tile rows, tile columns, grid x, grid y. */
int ao_nvfp4_linear_route(int kind, int64_t M, int64_t N, int64_t K, int32_t* out, int cap);
const char* ao_nvfp4_linear_kernel_name(int kind, int64_t M, int64_t N, int64_t K);
/* Measurement only (no reference counterpart: nvfp4_tensor.py:581-619 has one path): force the form of the calling thread's NVFP4
 * linears (0 the product route, 1 streaming, 2 tiled); the route query reports the forced form. */
int ao_nvfp4_linear_set_form(int form);

/* ---- NVFP4 training: the casts and the GEMM epilogue of prototype/moe_training/nvfp4_training (nvfp4_train_kernels.hip) --
 * The reference runs on sm100 only (Triton TMA and CuteDSL casts, cuBLAS scaled_mm).  The arithmetic is TransformerEngine's scale chain as
 * test/prototype/moe_training/nvfp4_training/nvfp4_reference.py states it -- csrc/quant_math.h ("NVFP4 training") -- and NOT
 * ao_nvfp4_quantize's: the block scale is rounded once and has no lower clamp, and the per-tensor amax is folded into an encode scale.
 * Codes are packed two a byte, element 2i in the low nibble; block scales are float8_e4m3fn bytes, ROW-MAJOR [rows][cols / 16] (what
 * ao_nvfp4_scaled_mm reads; the reference's 128 x 4 swizzle exists for cuBLAS).  sign_mask is the 16-point randomized Hadamard transform's
 * sign vector as a 16-bit mask: bit i set means s_i = -1.  NaN and Inf inputs are outside the contract.  Every per-tensor value is read
 * through a device pointer: no host read, every entry is graph-capturable.  Null pointers and bad shapes are rejected on the host before
 * any launch. */
/* Replaces triton_rht_amax / cutedsl_rht_amax (nvfp4_training/hadamard_amax_triton.py; nvfp4_reference.reference_rht_amax): x bf16 [M][N],
 * M and N multiples of 16 -> out2[0] = max|bf16(RHT(x^T))|, the transform along M in runs of 16 (0 and no transform when want_rht == 0),
 * out2[1] = max|x|, both fp32 on the device.  Clear, then an atomic max over the non-negative bit patterns.  x 16-byte, out2 4-byte
 * aligned. */
int ao_nvfp4_train_amax(const uint16_t* x, float* out2, int64_t M, int64_t N, uint32_t sign_mask, int want_rht, void* stream);
/* Replaces triton_rht_quantize_row_col / cutedsl_rht_quantize_row_col (nvfp4_training/hadamard_quantize_row_col_triton.py;
 * nvfp4_reference.reference_rht_quantize_row_col with layout="plain"): ONE read of x bf16 [M][N] gives the rowwise 1 x 16 cast of x
 * (row_q [M][N/2], row_s [M][N/16], under the amax amax2[1]) and the 1 x 16 cast of bf16(RHT(x^T)) written transposed (col_q [N][M/2],
 * col_s [N][M/16], under amax2[0]).  A null pair of outputs skips that direction.  sr_seed == NULL: round to nearest even.  Otherwise
 * stochastic rounding of BOTH outputs (this library's contract: Philox4x32-10 keyed by *sr_seed, counter (group of 8 codes, offset, stream),
 * stream 0 the row and 1 the column output, offsets *row_offset and *col_offset, their low 32 bits; quant_math.h), all three device int64
 * pointers.  The bytes depend on (seed, offset) only.  M and N multiples of 16, N > 0 (M == 0: OK, nothing launched).  x 16-byte, the
 * codes, the seed and the offsets 8-byte, amax2 4-byte aligned. */
int ao_nvfp4_train_quantize_row_col(const uint16_t* x, const float* amax2, uint32_t sign_mask, const int64_t* sr_seed, const int64_t* col_offset,
                                    const int64_t* row_offset, uint8_t* col_q, uint8_t* col_s, uint8_t* row_q, uint8_t* row_s, int64_t M, int64_t N,
                                    void* stream);
/* Replaces triton_weight_quantize_2d / cutedsl_weight_quantize_2d (nvfp4_training/quantize_2d_triton.py;
 * nvfp4_reference.reference_weight_quantize_2d with layout="plain"): w bf16 [N][K] under 16 x 16 block scales, no Hadamard transform,
 * round to nearest even, *amax = max|w| on the device.  q [N][K/2], s [N][K/16] with a block's scale replicated over its 16 rows; the same
 * read gives the cast of w^T, qt [K][N/2], st [K][N/16]: the same block scales and the codes of the same values.  N and K multiples of 16,
 * K > 0.  w 16-byte, the codes 8-byte, amax 4-byte aligned. */
int ao_nvfp4_train_quantize_weight_2d(const uint16_t* w, const float* amax, uint8_t* q, uint8_t* s, uint8_t* qt, uint8_t* st, int64_t N, int64_t K,
                                      void* stream);
/* Replaces torch.nn.functional.scaled_mm on e2m1 codes with BlockWise1x16 + TensorWise scales (nvfp4_training/nvfp4_linear.py:213-223,
 * :278-306): acc = sum_k (a_code a_s8)(b_code b_s8) in fp32;  out = bf16(acc (pa pb)), the product of the two fp32 scales taken in fp32,
 * ONE rounding, no bias.  (ao_nvfp4_linear rounds the accumulator and P to bf16 first: the inference reference's chain.)  The kernels
 * and the route of ao_nvfp4_linear (kind 1); a [M][K/2], a_scale [M][K/16], b [N][K/2], b_scale [N][K/16], pa and pb one fp32 each on the
 * device, both required.  Shapes and alignment as ao_nvfp4_linear. */
int ao_nvfp4_scaled_mm(const uint8_t* a, const uint8_t* a_scale, const float* pa, const uint8_t* b, const uint8_t* b_scale, const float* pb,
                       uint16_t* out, int64_t M, int64_t N, int64_t K, void* stream);

/* ---- NVFP4 grouped GEMM for MoE experts (nvfp4_kernels.hip) -------------------------------------------------------------
 * Replaces NVFP4Tensor's aten._grouped_mm (nvfp4_tensor.py:709-753) on 3-D weights with a per-expert [E, 1, 1] scale
 * (inference_workflow.py:309-319, nvfp4_tensor.py:830-834), which runs only through mslk or scaled_grouped_mm on sm100, and its portable
 * form _emulated_nvfp4_scaled_grouped_mm_2d_3d (prototype/moe_training/nvfp4_grouped_mm.py:62-116: both operands dequantized to bf16, then
 * torch._grouped_mm, 2 bytes a weight).  Token group e = rows [offs[e-1], offs[e]) (offs[-1] = 0) against expert e, the dense chain of
 * ao_nvfp4_wo_linear / ao_nvfp4_linear per output element, no bias (_grouped_mm has none):
 *   kind 0 (weight-only): w = bf16(f32(code) (pb[e] f32(s8)));  out = bf16(sum_k x w), fp32 sum, one rounding -- the reference's
 *     torch._grouped_mm(x, dequantize(bf16)^T, offs).
 *   kind 1 (codes x codes): acc = sum_k (a_code a_s8)(b_code b_s8) in fp32.  Neither pa nor pb: out = bf16(acc), the reference's emulated
 *     2d-3d function.  Otherwise t = bf16(acc);  out = bf16(f32(t) f32(bf16(P_e))), P_e = pa[e] pb[e] (fp32) or the one present: the
 *     dense entry's chain per group.  How sm100 applies the tensor-wise scales cannot be observed on this hardware, so this is the
 *     library's stated contract, as for ao_nvfp4_linear.
 * x bf16 [M_total][K] (kind 0; a and a_scale ignored) or a codes [M_total][K/2] with a_scale e4m3 [M_total][K/16] (kind 1; x ignored);
 * b codes [E][N][K/2]; b_scale e4m3 [E][N][K/16], row-major; pb fp32 [E] or NULL (per-expert weight scale); pa fp32 [E] or NULL
 * (per-group activation scale, kind 1 only: kind 0 refuses one); offs int32 [E], cumulative group ends, read on the device (no host sync);
 * out bf16 [M_total][N].  Rows past offs[E-1] are not written.  Empty groups are legal anywhere; group sizes need no alignment.  A group's
 * row range is clamped to [0, M_total] and a non-increasing pair of offs is an empty group, so a bad offs cannot address outside the
 * activation or out.  K parts are cut at multiples of 128 and added in part order: a launch is reproducible.
 * M_total >= 0 (0: OK, nothing launched), N >= 1 (ragged N masked), K a positive multiple of 16, 1 <= E <= 65535; M_total K and the
 * per-expert N K below 2^31 (the expert base is 64-bit pointer arithmetic: the whole b may pass 2^31 elements).  Alignment as the dense
 * entries (a per-expert stride cannot break the 16-byte row alignment for 16 | K); pa, pb and offs 4-byte.  Null pointers and bad shapes
 * are rejected on the host before any launch. */
/* The route keys on the mean group size ceil(M_total / E), all the host knows without a sync: nvfp4_grouped_stream_kernel up to this many
 * rows, nvfp4_grouped_tile_kernel beyond (one seam for both kinds).  It started at the 16 rows the blockwise float8 grouped GEMM fitted for
 * the same two-form structure; the sweep of tools/bench_nvfp4_grouped.py --sweep (each form forced over uniform groups of 2 .. 512 rows
 * on one EP-8 rank's DeepSeek-V3 and Qwen3-235B experts, both kinds, profiles/nvfp4_grouped.jsonl) moved it to 0: these tiles have 64
 * rows, not 128, and the tiled form was the faster one at EVERY swept group size, 2 rows included -- summed over the four shapes, both
 * kinds and fourteen group sizes the hand-over at 0 rows costs 37179 us, at 2 rows 37427, at 16 rows 38342, at 64 rows 43566.  So the
 * product route takes the tiled form for every M_total >= 1 and the streaming form is reached by the forced form only. */
#define AO_NVFP4_GROUPED_STREAM_MAX_ROWS 0
int ao_nvfp4_grouped_mm(int kind, const uint16_t* x, const uint8_t* a, const uint8_t* a_scale, const uint8_t* b, const uint8_t* b_scale,
                        const float* pa, const float* pb, const int32_t* offs, uint16_t* out, int64_t M_total, int64_t N, int64_t K, int64_t E,
                        void* stream);
/* Replaces per_tensor_amax_to_scale(amax(dim=(1, 2))) of the per-expert weight scale (inference_workflow.py:309-319) and the per-group
 * dynamic activation scale: x bf16 [M_total][K] -> out[e] = max|x[group e]| / 2688, the bits of ao_nvfp4_amax_scale on that group's rows
 * (NaN if the group holds one; an empty group gives 0).  No host read (capturable).  x 16-byte, out and offs 4-byte aligned. */
int ao_nvfp4_group_amax_scale(const uint16_t* x, const int32_t* offs, float* out, int64_t M_total, int64_t K, int64_t E, void* stream);
/* Replaces nvfp4_quantize (nvfp4_tensor.py:772-854) under a per-group scale: ao_nvfp4_quantize's bytes with row r cast under p[e] of the
 * group e that holds it (the first e with offs[e] > r).  Rows past offs[E-1] are not written.  p = NULL: ao_nvfp4_quantize on the rows
 * below offs[E-1].  The same two entries serve the weights: view [E][N][K] as [E N][K] with offs[e] = N (e + 1), which gives the reference's
 * bytes for to_nvfp4(w3d, per_tensor_scale=[E, 1, 1]) (nvfp4_quantize reshapes to [E, -1, 16] and broadcasts the scale, :830-834).  A zero
 * (or infinite) p[e] is outside the contract, as for ao_nvfp4_quantize: so is the dynamic per-group scale of an all-zero group. */
int ao_nvfp4_quantize_grouped(const uint16_t* x, const float* p, const int32_t* offs, uint8_t* q, uint8_t* scale_e4m3, int64_t M_total, int64_t K,
                              int64_t E, void* stream);
/* The route of ao_nvfp4_grouped_mm (host logic only; nvfp4_tensor.py:709-753 has one path, this library two forms): out[cap >= 7] = kernel
 * (0 = invalid kind or shape, or more than 65535 grid rows, 1 nvfp4_grouped_stream_kernel, 2 nvfp4_grouped_tile_kernel), waves per
 * workgroup, m-tiles of 16 per pass or workgroup, tile rows, tile columns, grid x, grid y (stream: E; tile: ceil(M_total / 64) + E, the
 * host's upper bound on the tile count). */
int ao_nvfp4_grouped_mm_route(int kind, int64_t M_total, int64_t N, int64_t K, int64_t E, int32_t* out, int cap);
/* "nvfp4_grouped_stream_kernel", "nvfp4_grouped_tile_kernel" or "invalid": the kernel of that route. */
const char* ao_nvfp4_grouped_mm_kernel_name(int kind, int64_t M_total, int64_t N, int64_t K, int64_t E);
/* Measurement only (no reference counterpart): force the form of the calling thread's NVFP4 grouped GEMMs (0 the product route,
 * 1 streaming, 2 tiled); the route queries report the forced form. */
int ao_nvfp4_grouped_mm_set_form(int form);

/* ---- quantization-aware training: the fake quantizers of torchao.quantization.qat, one launch per direction ----------
 * bf16 in, bf16 out, fp32 in between in the reference's order; every division correctly rounded; the only rounding to bf16 is the last.
 * The backward entries take only the forward's INPUT and the incoming gradient: the range, the scale and the codes are made again, no
 * mask is stored.  No atomics: the same bytes every launch.  No allocation, no synchronisation: capturable in a graph.  Pointers
 * 16-byte aligned. */

/* Replaces Int4WeightFakeQuantizer._bf16_activations_forward (qat/fake_quantizer.py:167-187), some fifteen tensor ops: per group of
 * group_size along K,  M = max, m = min, s = max(M - m, 1e-6) / 15,  q = clamp(rint((w - m) / s), 0, 15),
 * out = bf16((q - 8) s + (m + 8 s)) -- the value bf16-dequantised codes of ao_int4_plain_quantize stand for.
 * w, out bf16 [N][K].  group_size in {32, 64, 128, 256}, K % group_size == 0 (K % 128 is NOT required); N == 0 launches nothing. */
int ao_qat_int4_fake_quantize(const uint16_t* w, uint16_t* out, int64_t N, int64_t K, int group_size, void* stream);
/* Replaces autograd through the same lines (qat/fake_quantizer.py:167-187; _Round, qat/utils.py, is straight-through): with G = grad_out,
 * t the unclamped quotient, c = 1 where 0 <= rint(t) <= 15,
 *   ds = sum G (q - c t),  dm = sum G (1 - c),  dr = ds / 15 where M - m >= 1e-6 else 0,
 *   grad_w = bf16(G c + [w = M] dr / #{w = M} + [w = m] (dm - dr) / #{w = m})       (sums over the group; ties share evenly) */
int ao_qat_int4_fake_quantize_bwd(const uint16_t* w, const uint16_t* grad_out, uint16_t* grad_w, int64_t N, int64_t K, int group_size,
                                  void* stream);
/* Replaces Float8FakeQuantizer.forward with PerRow() and float8_e4m3fn (qat/fake_quantizer.py:84-98 over _choose_scale_float8,
 * _quantize_affine_float8, _dequantize_affine_float8, quant_primitives.py:2173-2304): per row,
 *   a = clamp(max|x|, lb, ub) as bf16 values (the reference clamps the bf16 amax),  s = f32(bf16(a / 448)),
 *   out = bf16(f32(e4m3_rne(clamp(f32(x) / s, -448, 448))) s)
 * lb, ub: hp_value_lb / hp_value_ub; -INFINITY / +INFINITY when absent.  A row whose clamped amax is 0 is NaN (0 / 0), as in the reference,
 * written as 0xFFFF.  x, out bf16 [R][C], C % 16 == 0; R == 0 launches nothing.  Rows of up to 16384 elements stay in registers between
 * the amax and the cast; longer rows are walked twice. */
int ao_qat_fp8_fake_quantize_rowwise(const uint16_t* x, uint16_t* out, int64_t R, int64_t C, float lb, float ub, void* stream);
/* The gradient of that chain (qat/fake_quantizer.py:84-98, quant_primitives.py:2173-2304) with EVERY cast straight-through -- not the
 * reference's autograd, which rounds the incoming gradient to e4m3.  With t = f32(x) / s, c = 1 where |t| <= 448:
 *   ds = sum G (q - c t),  da = ds / 448 where lb <= max|x| <= ub else 0,
 *   grad_x = bf16(G c + [|x| = max|x|] sign(x) da / #{|x| = max|x|})                 (sums over the row; ties share evenly) */
int ao_qat_fp8_fake_quantize_rowwise_bwd(const uint16_t* x, const uint16_t* grad_out, uint16_t* grad_x, int64_t R, int64_t C, float lb,
                                         float ub, void* stream);

/* ---- NF4 (QLoRA) weights: NF4Tensor of quantization/quantize_/workflows/nf4/nf4_tensor.py (nf4_kernels.hip) -------------
 * A flattened bf16 tensor of numel elements in blocks of block_size (32, 64 or 128); scaler blocks of scaler_block_size (a power of two)
 * consecutive blocks; numel a multiple of block_size x scaler_block_size, below 2^31.  The tensor's fields as the reference stores them:
 * codes uint8 [numel / 2] (quantized_data, element 2i in the HIGH nibble), scalers int8 [numel / block_size] (quantized_scalers), factors
 * bf16 [numel / (block_size x scaler_block_size)] (quantization_factor), mean one bf16 on the device (scaler_mean).  The arithmetic is
 * stated once, in csrc/quant_math.h ("NF4"), and gives the reference's bytes.  Anything else is rejected on the host before any launch;
 * no allocation, no synchronisation: capturable in a graph. */
/* Replaces get_block_absmax (nf4_tensor.py:560-577): absmax[b] = max |x| over block b, NaN if the block holds one. */
int ao_nf4_block_absmax(const uint16_t* x, uint16_t* absmax, int64_t numel, int block_size, void* stream);
/* Replaces the rest of NF4Tensor.from_tensor (nf4_tensor.py:649-718: double_quantize_scalers :721-778 and convert_to_norm_float_weight
 * :806-843 with quantize_tensor_nearest :874-880) in ONE launch, given absmax and its mean -- bf16(absmax.mean()), the only value that
 * depends on a summation order, which the caller takes from torch on the device.  A scaler block whose centred scalers are all zero has an
 * infinite factor and NaN products, whose int8 the reference leaves undefined: 0 here. */
int ao_nf4_quantize(const uint16_t* x, const uint16_t* absmax, const uint16_t* mean, uint8_t* codes, int8_t* scalers, uint16_t* factors,
                    int64_t numel, int block_size, int64_t scaler_block_size, void* stream);
/* Replaces NF4Tensor.get_original_weight (nf4_tensor.py:845-871 with dequantize_scalers :780-803): w bf16 [numel], 16-byte aligned. */
int ao_nf4_dequantize(const uint8_t* codes, const int8_t* scalers, const uint16_t* factors, const uint16_t* mean, uint16_t* w, int64_t numel,
                      int block_size, int64_t scaler_block_size, void* stream);
/* Replaces LinearNF4.forward (nf4_tensor.py:1053-1058: F.linear(input, weight.to(input.dtype))) at decode row counts, the weight-streaming
 * form only: x bf16 [M][K] times the fields of W [N][K] -> out bf16 [M][N] = bf16(sum_k x w), w the bits of ao_nf4_dequantize, fp32
 * accumulation, no bias (the reference adds it outside).  The weight is read once, straight from the fields.  K % block_size == 0 (blocks
 * inside rows); x and codes 16-byte aligned; M == 0 launches nothing.  A shape whose route is "not fused" is an error here. */
int ao_nf4_linear(const uint16_t* x, const uint8_t* codes, const int8_t* scalers, const uint16_t* factors, const uint16_t* mean, uint16_t* out,
                  int64_t M, int64_t N, int64_t K, int block_size, int64_t scaler_block_size, void* stream);
/* The route of LinearNF4.forward (nf4_tensor.py:1053-1058 has one path; host logic only): out[cap >= 7] = kernel (1 nf4_stream_kernel;
 * 0 not fused -- above the row count up to which the fused form wins, or a shape ao_nf4_linear does not take: ao_nf4_dequantize, then a
 * bf16 GEMM), waves, m-tiles, tile rows, tile columns, grid x, grid y. */
int ao_nf4_linear_route(int64_t M, int64_t N, int64_t K, int block_size, int64_t scaler_block_size, int32_t* out, int cap);
/* "nf4_stream_kernel" or "not fused": the kernel of that route. */
const char* ao_nf4_linear_kernel_name(int64_t M, int64_t N, int64_t K, int block_size, int64_t scaler_block_size);
/* Measurement only (no reference counterpart): 1 forces the stream kernel at any M for the calling thread, 0 restores the route. */
int ao_nf4_linear_set_form(int form);

/* ---- Low-bit optimizers: torchao/optim's block-quantized Adam moments and its single_param_adam (adam.py:163-209) ---------------------------
 * A state is taken flat in blocks of block_size elements (a power of two, 64 .. 2048, n a multiple of it): codes (uint8 one an element;
 * 4-bit: two a byte, element 2i in the high nibble; fp8: e4m3fn bytes), scale fp32 [n / block_size], and for the table formats the state's
 * own qmap (fp32 [256] or [16], on the device: no kernel holds a table).  The arithmetic is stated once, in csrc/quant_math.h ("low-bit
 * optimizer states"), and gives the bytes of the reference's eager CPU run.  Data pointers 16-byte aligned.  No allocation, no
 * synchronisation; anything else is rejected on the host before any launch. */
enum {
  AO_OPTIM_Q8_SIGNED = 0,
  AO_OPTIM_Q8_UNSIGNED = 1,
  AO_OPTIM_Q4_SIGNED = 2,
  AO_OPTIM_Q4_UNSIGNED = 3,
  AO_OPTIM_FP8 = 4,
  AO_OPTIM_PLAIN = 5 /* ao_optim_adam_step only: moments in the parameter's dtype, any n */
};
/* The scalars of one step, computed on the host with the torch CPU operations the reference runs on its 0-dim tensors. */
typedef struct {
  float lr;
  float lr_wd;                 /* lr * weight_decay */
  float wd;
  float one_minus_beta1;       /* fp32(1 - beta1), the Python double rounded */
  float one_minus_beta2;
  float bias_correction1;      /* 1 - beta1^step */
  float sqrt_bias_correction2; /* sqrt(1 - beta2^step) */
  float eps;
} ao_optim_scalars;
/* Replaces the subclasses' copy_ from a float tensor (subclass_8bit.py:137-141, subclass_4bit.py:155-159, subclass_fp8.py:115-118): src
 * fp32 or bf16 [n] -> codes, scale.  The signed and the unsigned format of a width differ in the qmap alone (null for fp8). */
int ao_optim_quantize(const void* src, int src_bf16, void* codes, float* scale, const float* qmap, int64_t n, int block_size, int format,
                      void* stream);
/* Replaces dequantize() (subclass_8bit.py:97-101, subclass_4bit.py:107-112, subclass_fp8.py:77-83): dst fp32 [n], or that rounded to bf16. */
int ao_optim_dequantize(const void* codes, const float* scale, const float* qmap, void* dst, int dst_bf16, int64_t n, int block_size,
                        int format, void* stream);
/* Replaces single_param_adam for ONE parameter in ONE launch: p and grad [n] of one dtype (bf16 or fp32), updated in place with the moments'
 * codes and scales.  format: the first moment's (AO_OPTIM_Q8_SIGNED, AO_OPTIM_Q4_SIGNED, AO_OPTIM_FP8) or AO_OPTIM_PLAIN, where m_codes /
 * v_codes / vmax_codes are the moments themselves in p's dtype and scales and qmaps are null.  vmax_codes null: no amsgrad.  sr != 0 (bf16 p
 * only): p is rounded stochastically from (seed, step, param_index, element).  max_workgroups > 0 caps the grid (0: the default of
 * ao_optim_grid); the bytes never depend on it.  The scalars go by value and change every step: a captured launch would replay stale ones. */
int ao_optim_adam_step(void* p, const void* grad, int bf16, void* m_codes, float* m_scale, const float* m_qmap, void* v_codes, float* v_scale,
                       const float* v_qmap, void* vmax_codes, float* vmax_scale, const float* vmax_qmap, int format, int64_t n, int block_size,
                       const ao_optim_scalars* scalars, int is_adamw, int sr, int64_t seed, int64_t step, int64_t param_index,
                       int max_workgroups, void* stream);
/* The grid rule of the three entries above (host logic only): out[0] = elements a workgroup takes per trip of its loop (a multiple of every
 * block size), out[1] = trips in all (tiles), out[2] = workgroups launched = min(tiles, max_workgroups or the default cap). */
int ao_optim_grid(int64_t n, int max_workgroups, int64_t* out);

/* ---- GPTQ (torchao/prototype/gptq) ------------------------------------------------------------------------------------------------------------
 * Replaces the column loop of gptq_quantize for ONE GPTQ block (prototype/gptq/api.py:446-532: per column a dozen eager launches on [N, 1]
 * slices) and the final re-quantization of that block's columns (:537-569), in ONE launch.  The arithmetic is stated once, at the head of
 * csrc/gptq_kernels.hip: every step one fp32 operation rounded once, no fma, IEEE division, rint to even; bf16 weights round at every update.
 *   W       [N][K] bf16 (w_bf16 != 0) or fp32, updated IN PLACE in columns [k0, k0 + block_cols)
 *   Hinv    fp32 [K][K], the upper Cholesky factor api.py:400-403 calls Hinv; rows and columns [k0, k0 + block_cols) are read; 16-byte aligned
 *   Err     fp32 [N][block_cols], written: err of every column, the operand of the host's lazy batch update (:530-532)
 *   AO_GPTQ_INT4   (_int4_row_quantize_zp_precomputed_qparams / _int4_row_dequantize_zp, api.py:167-221; group_size 32 | 64 | 128 | 256)
 *                  qdata uint8 [N][K/2], even k in the low nibble; scale / zero_point [K/g][N] in W's dtype (rounded on store; fp32 inside
 *                  the loop: PARITY UNPINNED, mslk is un-vendored); aux unused
 *   AO_GPTQ_NVFP4  (_nvfp4_with_precalculated_scales_qdq / _q, api.py:224-274; nvfp4_quantize's block scales, nvfp4_tensor.py:772-854)
 *                  qdata uint8 [N][K/2], scale e4m3 bytes [N][K/16] row-major, aux = the fp32 per-tensor scale (one element, on the device),
 *                  group_size 16; zero_point unused
 *   AO_GPTQ_INT8   (Int8Tensor.from_hp(scale=) + dequantize(float), int8_tensor.py:176-259) qdata int8 [N][K], aux = fp32 [N] row scales
 *                  (given, not measured: see DESIGN.md for the deviation from api.py:471-478); scale, zero_point and group_size unused
 * block_cols <= 256 (the block's tile of W and Err stay in LDS), a multiple of 16 and of the group size, as are k0 and K; any N. */
enum { AO_GPTQ_INT4 = 0, AO_GPTQ_INT8 = 1, AO_GPTQ_NVFP4 = 2 };
int ao_gptq_block(void* W, int w_bf16, const float* Hinv, float* Err, int format, int group_size, void* qdata, void* scale, void* zero_point,
                  const float* aux, int64_t N, int64_t K, int64_t k0, int64_t block_cols, void* stream);

/* ---- AWQ (torchao/prototype/awq) --------------------------------------------------------------------------------------------------------------
 * The weight's side of AWQObserver.calculate_qparams' search loop (prototype/awq/core.py:70-86: per ratio a scaled weight, the whole int4
 * quantize_ handler and two F.linear over every calibration token), for R candidate scale vectors in ONE launch that reads W once.  Per
 * ratio r, row n and group of group_size columns, every step one fp32 operation rounded once, no fma, IEEE division, rint to even:
 *   ws = bf16(W[n][k] * S[r][k]);  M, m = max, min of ws over the group;  s = max(M - m, 1e-6) / 15;  z = m + 8 s
 *   q  = clamp(rint((ws - m) / s), 0, 15) - 8                          (the codes of ao_int4_plain_quantize)
 *   dq = bf16(f32(bf16(q * f32(bf16(s)))) + f32(bf16(z)))              (Int4Tensor.from_hp(W * S[r]).dequantize(), byte for byte)
 *   D[r][n][k] = f32(W[n][k]) - f32(dq) / f32(S[r][k])
 * so that the reference's loss mean((X W^T - (X / S[r]) Wq^T)^2) is tr(D[r] G D[r]^T) / (rows N) with G = X^T X (the host's matmul).
 *   W bf16 [N][K];  S bf16 [R][K], every entry finite and > 0;  D fp32 [R][N][K], exactly that size;  all 16-byte aligned.
 * group_size in {32, 64, 128, 256}, K % group_size == 0 (K % 128 is NOT required); any N and R; N == 0 or R == 0 launches nothing.  No LDS,
 * no atomics: the same bytes every launch.  No allocation, no synchronisation: capturable in a graph. */
int ao_awq_scaled_error(const uint16_t* W, const uint16_t* S, float* D, int64_t N, int64_t K, int64_t R, int group_size, void* stream);

/* ---- SmoothQuant (torchao/prototype/smoothquant) ---------------------------------------------------------------------------------------------
 * Calibration (prototype/smoothquant/core.py:41-75, 162-206), as running reductions that never hold more than their state:
 *   ao_sq_col_absmax_update     state[k] = max(state[k], max_m |x[m][k]|)                         x bf16 [M][K], state fp32 [K]
 *   ao_sq_smoothed_amax_update  amax[0]  = max(amax[0], max_mk |bf16(f32(x[m][k]) / f32(s[k]))|)   s bf16 [K] (> 0, finite), amax fp32 [1]
 * Both fold with an integer atomic max on the bit pattern of non-negative floats: exact, independent of the order of arrival, the same bytes
 * every launch.  The state must hold non-negative floats (zeros before the first update); -0.0 counts as 0; IEEE division; NaN / Inf inputs
 * are outside the contract.
 * Run time: the int8 activation casts with the activation pre-scale folded in, t = bf16(f32(x[m][k]) * f32(pre[k])) (the bf16 tensor op
 * `x * act_pre_scale`: the product is exact in fp32, so one rounding), pre bf16 [K]:
 *   ao_int8_quantize_rowwise_prescaled     ao_int8_quantize_rowwise on t:  q int8 [M][K], scale fp32 [M]
 *   ao_int8_quantize_tensorwise_prescaled  one amax over all of t (Int8Tensor.from_hp(t, PerTensor())): `amax` fp32 [1] is a work buffer the
 *                                          call zeroes and fills; scale fp32 [M], every entry the tensor's scale
 *   ao_int8_quantize_static_prescaled      ao_int8_quantize_static on t (given scale / zero-point, one per tensor or, per_row != 0, per row)
 * Byte for byte what the unscaled cast gives on `x * pre` computed by a bf16 multiply.  t is never written to memory.
 * All: K % 8 == 0, x / s / pre 16-byte aligned, M == 0 launches nothing.  No allocation, no synchronisation: capturable in a graph. */
int ao_sq_col_absmax_update(const uint16_t* x, float* state, int64_t M, int64_t K, void* stream);
int ao_sq_smoothed_amax_update(const uint16_t* x, const uint16_t* s, float* amax, int64_t M, int64_t K, void* stream);
int ao_int8_quantize_rowwise_prescaled(const uint16_t* x, const uint16_t* pre, int8_t* q, float* scale, int64_t M, int64_t K, void* stream);
int ao_int8_quantize_tensorwise_prescaled(const uint16_t* x, const uint16_t* pre, float* amax, int8_t* q, float* scale, int64_t M, int64_t K,
                                          void* stream);
int ao_int8_quantize_static_prescaled(const uint16_t* x, const uint16_t* pre, const float* scale, const int8_t* zero_point, int per_row,
                                      int8_t* q, int64_t M, int64_t K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AO_MI355_H */
