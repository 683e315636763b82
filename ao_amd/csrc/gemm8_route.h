// Host only: which kernel an 8-bit GEMM entry point launches for a shape, and with what launch shape.
// gemm8_route (gemm8_kernels.hip) is the one function that decides: the entry points launch what it returns, and the introspection
// queries (ao_gemm8_kernel_name / ao_gemm8_plan / ao_gemm8_plan_rows) report what it returns for the product (Gemm8Force{}).
// grouped8_route (rb8_kernels.hip) does the same for the grouped entry points (ao_fp8_grouped_mm, ao_mxfp8_grouped_mm and its fused-cast /
// pair forms; ao_grouped8_route reports it).
// The band rules it is built from are pure functions of the shape and the forced codes, defined next to their kernels.
// The A/B knobs that change no route are read by the launchers from gemm8_force(): rb8_kernel's wave arrangement (variant 103) and probe
// bits (tuning key 5), gemm8_p8(h)'s group rows (key 4), the MX stream-K meeting (key 9).
#pragma once
#include <stdint.h>

namespace ao {

// ao_int8_scaled_mm, ao_fp8_scaled_mm, ao_int8_int_mm, ao_fp8_mm_f32, ao_int8_dynamic_linear, ao_fp8_dynamic_linear
enum class Gemm8Entry { Int8Scaled, Fp8Scaled, Int32Raw, Fp8Raw, Int8Dyn, Fp8Dyn };

// the kernels by the names ao_gemm8_kernel_name reports (kGemm8KernelNames, gemm8_kernels.hip); Dma256x128 / Dma256x256w4 (4 waves of
// 128 x 128) only under variants 4 / 16, RegStage where K % 128 != 0 or under variant 1
enum class Gemm8Kernel { Invalid, Dec8, Mid8, Stream8, Rb8, P8h, P8, P8p, Dma128, Dma256, Dma256x128, Dma256x256w4, RegStage, Dyn8 };

struct Dec8Shape {
  int waves, depth;
  bool loop;           // K does not factor: the ring is refilled in a loop (depth 4)
  bool half = false;   // half-line loads, no LDS transposition (variant 290)
  bool rows8 = false;  // 8-row tiles
};

struct Mid8Plan {
  int mt, split;
};

// tile_rows / tile_cols / k_parts: what ao_gemm8_plan(_rows) report -- rb8: slab rows, column-tile width, K parts; p8h: 256 x 128 and its
// K parts; the tiled GEMMs their tile and one part; the per-tile streaming kernels (dec8 / mid8 / stream8 / dyn8) 16 x 16 and one part
// (their launch shape is in dec / mid)
struct Gemm8Route {
  Gemm8Kernel kernel = Gemm8Kernel::Invalid;
  int tile_rows = 16, tile_cols = 16, k_parts = 1;
  Dec8Shape dec{};
  Mid8Plan mid{};
};

// Every override ao_gemm8_set_variant / ao_gemm8_set_tuning set (include/ao_mi355.h).  Default-constructed: the product dispatch.
struct Gemm8Force {
  // ao_gemm8_set_variant
  bool regstage = false;    // 1: the register-staged tile kernel wherever a tiled GEMM runs
  bool tiled_only = false;  // 100: never a weight-streaming kernel
  int tile = 0;             // 2 / 4 / 8 / 16 / 32 / 33: that tiled GEMM form
  int rb = 0;               // the rowwise weight-streaming kernel: 1 never (100, explicit tile variants), 2 always (101), 3 always + 64 columns (102)
  bool rb8_1x8 = false;     // 103: its round-3 wave arrangement (1 x 8)
  int mx = 0;               // MXFP8 grouped mm: 2 never the LDS-staged kernels (111); 1 (110) is the product route, kept so old scripts run
  bool mx_stream = true;    // 113 (false): decode-size groups take one workgroup per tile instead of the stream-K kernel
  bool mx_quad = true;      // 129 (false): the stream-K kernel's per-step-scales form on every K
  int dec8 = 0;             // 200 .. 299: dec8_kernel's forms (dec8_plan)
  int mid8 = 0;             // 300 .. 329: mid8_kernel's forms (mid8_plan)
  // ao_gemm8_set_tuning keys 1 .. 7 and 9 (key 8 is accepted and ignored: it sets nothing here and does not mark the thread as overridden)
  int rb8_bn = 0, rb8_split = 0, rb8_bm = 0, p8_group_rows = 0, rb8_ablate = 0, p8_persist = 0, p8_split = 0, mx_proto = 0;
};

// the calling thread's overrides (gemm8_kernels.hip)
const Gemm8Force& gemm8_force();

// aligned: row / column scales and output 16-byte aligned, bias 4-byte aligned (the persistent 256 x 256 form needs it)
Gemm8Route gemm8_route(Gemm8Entry entry, int64_t M, int64_t N, int64_t K, bool aligned, const Gemm8Force& f);

// ao_fp8_grouped_mm, ao_mxfp8_grouped_mm, ao_mxfp8_grouped_mm_dyn, ao_mxfp8_grouped_mm_dyn_pair, ao_mxfp8_grouped_mm_pair
enum class Grouped8Entry { Fp8Rowwise, Mx, MxDyn, MxDynPair, MxPair };

// rb8_kernel (RB8_FP8_GROUPED / RB8_MX), mx_stream_kernel (stream-K), mx_grouped_kernel, stream8_kernel<S8_MX>
enum class Grouped8Kernel { Invalid, Rb8, MxStream, MxGrouped, Stream8 };

// The template arguments and launch shape of a grouped launch -- rb8: <waves, mt, slim, qs> over slabs of slab_rows rows, `slabs` per group;
// mx_stream: <waves, sw, qs, cast>; mx_grouped: <mt, tn>; stream8: <mt>
struct Grouped8Route {
  Grouped8Kernel kernel = Grouped8Kernel::Invalid;
  int waves = 0, mt = 0, slim = 0, qs = 0, sw = 0, cast = 0, tn = 0, slab_rows = 0, slabs = 0;
};

// The one decision of the grouped entry points, and the only reader of the MX forcing codes (variants 110 / 111 / 113 / 129, tuning key 3).
// aligned: every pointer the per-4-step-scale (QS = 4) and stream-K forms read is 16-byte aligned; scaling_mode: the fused cast's
// (AO_MX_SCALE_FLOOR / _RCEIL).  Invalid: the entry refuses the shape.
Grouped8Route grouped8_route(Grouped8Entry entry, int64_t M_total, int64_t N, int64_t K, int64_t E, bool have_offs, bool aligned, int scaling_mode,
                             const Gemm8Force& f);

// ---- band rules (pure) ----
bool dec8_plan(int64_t M, int64_t N, int64_t K, int mode, Dec8Shape* shape);  // dec8_kernels.hip (mode: Gemm8Force::dec8)
bool mid8_plan(int64_t M, int64_t N, int64_t K, int mode, Mid8Plan* plan);    // mid8_kernels.hip (mode: Gemm8Force::mid8)
bool rb8_preferred(int64_t M, int64_t N, int64_t K, int force);               // rb8_kernels.hip (force: Gemm8Force::rb)
bool rb8_small_m_preferred(int64_t M, int64_t N, int64_t K, int force);
void rb8_launch_plan(int64_t M, int64_t N, int64_t K, const Gemm8Force& f, int* bm, int* bn, int* split);
bool gemm8_p8_fits(int64_t M, int64_t N, int64_t K);  // gemm8_p8_kernels.hip
bool gemm8_p8h_band(int64_t M, int64_t N, int64_t K);
int gemm8_p8h_parts(int64_t M, int64_t N, int64_t K, int forced);
bool gemm8_p8_persistent_shape(int64_t M, int64_t N, int64_t K);

}  // namespace ao
