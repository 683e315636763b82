// Host only: which kernel an 8-bit GEMM entry point launches for a shape, and with what launch shape.
// gemm8_route (gemm8_kernels.hip) is the one function that decides: the entry points launch what it returns, and the introspection
// queries (ao_gemm8_kernel_name / ao_gemm8_plan / ao_gemm8_plan_rows) report what it returns for the product (Gemm8Force{}).
// The band rules it is built from are pure functions of the shape and the forced codes, defined next to their kernels.
// The A/B knobs that change no route are read by the launchers from gemm8_force(): rb8_kernel's wave arrangement (variant 103) and probe
// bits (tuning key 5), gemm8_p8(h)'s group rows (key 4), the laboratory loop forms of gemm8_p8h (key 8), the MX stream-K meeting (key 9).
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
  int mx = 0;               // MXFP8 grouped mm: 1 always the LDS-staged kernels (110), 2 never (111)
  bool mx_stream = true;    // 113 (false): decode-size groups take one workgroup per tile instead of the stream-K kernel
  bool mx_quad = true;      // 129 (false): the stream-K kernel's per-step-scales form on every K
  int dec8 = 0;             // 200 .. 299: dec8_kernel's forms (dec8_plan)
  int mid8 = 0;             // 300 .. 329: mid8_kernel's forms (mid8_plan)
  // ao_gemm8_set_tuning keys 1 .. 9
  int rb8_bn = 0, rb8_split = 0, rb8_bm = 0, p8_group_rows = 0, rb8_ablate = 0, p8_persist = 0, p8_split = 0, p8h_form = 0, mx_proto = 0;
};

// the calling thread's overrides (gemm8_kernels.hip)
const Gemm8Force& gemm8_force();

// aligned: row / column scales and output 16-byte aligned, bias 4-byte aligned (the persistent 256 x 256 form needs it)
Gemm8Route gemm8_route(Gemm8Entry entry, int64_t M, int64_t N, int64_t K, bool aligned, const Gemm8Force& f);

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
