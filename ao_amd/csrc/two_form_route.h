// Host only: the frame of a linear family that has a weight-streaming form and an LDS-tiled form -- the MX dense linears
// (mx_linear_kernels.hip), the int8 / float8 weight-only linears (wo8_kernels.hip), the blockwise float8 linears, dense and grouped
// (fp8_block_kernels.hip), and the NVFP4 linears, dense and grouped (nvfp4_kernels.hip).  A family keeps what it measured or what its
// kernels need: its shape check, the row counts at which it hands over from the stream form to the tiled form, the tile edge of its
// tiled form, its own thread-local forced form (ao_*_set_form), its argument structs, its kernels, the pointer and alignment checks
// of its entries and the choice of template arguments.  Here, once:
//   the route: the plan of either form and the grid-row cap (two_form_route), and the grouped route on the mean group size with its
//     + E grid rows (grouped_two_form_route);
//   the bodies of the exports: ao_*_route (route_export, the seven fields of write_route), ao_*_kernel_name (route_kernel_name) and
//     ao_*_set_form (set_forced_form);
//   the launches: the compile-time (m-tiles, waves) pair of a stream-form launch (with_stream_form, launch_stream_form) and the
//     tiled form's launch with or without dynamic LDS (launch_tile_form).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "common.h"

namespace ao {

// the ao_*_route exports write these seven fields, in this order (write_route)
struct TwoFormRoute {
  int kernel = 0;  // 0 invalid, 1 the stream form, 2 the tiled form
  int waves = 0;   // waves per workgroup
  int mt = 0;      // m-tiles of 16 per workgroup
  int tile_m = 0, tile_n = 0;
  int grid_x = 0, grid_y = 0;
};

inline void write_route(const TwoFormRoute& r, int32_t* out) {
  const int32_t v[7] = {r.kernel, r.waves, r.mt, r.tile_m, r.tile_n, r.grid_x, r.grid_y};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
}

// The stream form: a workgroup owns 16 columns and up to 64 rows (1 / 2 / 4 m-tiles by M; more rows add grid rows) and splits K over
// its waves in 128-k steps.
inline TwoFormRoute stream_form_plan(int64_t M, int64_t N, int64_t K) {
  TwoFormRoute r;
  const int64_t ntiles = (N + 15) / 16;
  const int64_t ksteps = (K + 127) / 128;
  r.kernel = 1;
  r.mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  // enough waves in flight to cover HBM latency on 256 CUs: fewer column tiles, more K parts per tile; no wave without a k step
  int w = ntiles >= 1024 ? 4 : (ntiles >= 256 ? 8 : 16);
  if (r.mt == 4 && w > 8) w = 8;  // the meeting buffer: waves x m-tiles x 1 KiB of static LDS
  while (w > 1 && w > ksteps) w >>= 1;
  r.waves = w;
  r.tile_m = 16 * r.mt;
  r.tile_n = 16;
  r.grid_x = (int)ntiles;
  r.grid_y = (int)std::max<int64_t>(1, (M + r.tile_m - 1) / r.tile_m);
  return r;
}

// The tiled form: four waves on square output tiles of the family's edge.  (No rows, no grid rows: M = 0 is never launched.)
inline TwoFormRoute tiled_form_plan(int64_t M, int64_t N, int edge) {
  TwoFormRoute r;
  r.kernel = 2;
  r.waves = 4;
  r.mt = 4;
  r.tile_m = edge;
  r.tile_n = edge;
  r.grid_x = (int)((N + edge - 1) / edge);
  r.grid_y = (int)((M + edge - 1) / edge);
  return r;
}

// form: 1 stream, 2 tiled (the family's seam or its forced form picked it).  Rows ride on the grid's y dimension, which ends at 65535.
inline TwoFormRoute two_form_route(int form, int64_t M, int64_t N, int64_t K, int tile_edge) {
  TwoFormRoute r = form == 1 ? stream_form_plan(M, N, K) : tiled_form_plan(M, N, tile_edge);
  if (r.grid_y > 65535) r.kernel = 0;
  return r;
}

// The grouped (MoE experts) route.  Without a sync the host knows only M_total and E, so the family's seam meets the mean group size
// ceil(M_total / E).  The stream form: grid (ceil(N / 16), E), m-tiles and waves of the stream plan at the mean size.  The tiled form:
// grid (ceil(N / edge), ceil(M_total / edge) + E), a group's last tile being ragged.  forced: the family's forced form, 0 for its seam.
inline TwoFormRoute grouped_two_form_route(int forced, int seam, int64_t M_total, int64_t N, int64_t K, int64_t E, int tile_edge) {
  const int64_t mean = (M_total + E - 1) / E;
  const int form = forced != 0 ? forced : (mean <= seam ? 1 : 2);
  TwoFormRoute r = two_form_route(form, form == 1 ? mean : M_total, N, K, tile_edge);
  if (r.kernel == 0) return TwoFormRoute{};
  const int64_t gy = form == 1 ? E : (int64_t)r.grid_y + E;
  if (gy > 65535) return TwoFormRoute{};
  r.grid_y = (int)gy;
  return r;
}

// ---- the bodies of a family's exports; fn: the entry's own name, as its errors carry it ---------------------------------------------
inline int route_export(const char* fn, const TwoFormRoute& r, int32_t* out, int cap) {
  AO_REQUIRE_PTR_FN(fn, out);
  AO_REQUIRE(cap >= 7, "%s: cap must be >= 7, got %d", fn, cap);
  write_route(r, out);
  return AO_OK;
}

inline const char* route_kernel_name(const TwoFormRoute& r, const char* stream, const char* tile) {
  return r.kernel == 1 ? stream : (r.kernel == 2 ? tile : "invalid");
}

inline int set_forced_form(const char* fn, int form, int& forced) {
  AO_REQUIRE(form >= 0 && form <= 2, "%s: form must be 0 (route), 1 (stream) or 2 (tile), got %d", fn, form);
  forced = form;
  return AO_OK;
}

// Calls launch(m-tiles, waves) with the stream-form route's pair as std::integral_constants, for the kernel templates of a family; a
// pair stream_form_plan never produces is an error.  MT4_W16: whether the family has a kernel of 4 m-tiles x 16 waves (the plan caps
// 4 m-tiles at 8 waves, so nothing reaches it; a family whose meeting buffer would pass the static LDS limit there must not compile it).
template <bool MT4_W16, typename Launch>
int with_stream_form(const char* kernel, const TwoFormRoute& r, Launch&& launch) {
  auto waves = [&](auto mt) {
    switch (r.waves) {
      case 1: launch(mt, std::integral_constant<int, 1>{}); return true;
      case 2: launch(mt, std::integral_constant<int, 2>{}); return true;
      case 4: launch(mt, std::integral_constant<int, 4>{}); return true;
      case 8: launch(mt, std::integral_constant<int, 8>{}); return true;
      case 16:
        if constexpr (MT4_W16 || decltype(mt)::value <= 2) {
          launch(mt, std::integral_constant<int, 16>{});
          return true;
        }
        [[fallthrough]];
      default: return false;
    }
  };
  const bool found = r.mt == 1   ? waves(std::integral_constant<int, 1>{})
                     : r.mt == 2 ? waves(std::integral_constant<int, 2>{})
                     : r.mt == 4 ? waves(std::integral_constant<int, 4>{})
                                 : false;
  if (!found) {
    set_error("%s: no instantiation for %d m-tiles x %d waves", kernel, r.mt, r.waves);
    return AO_ERR_INVALID_ARGUMENT;
  }
  return AO_OK;
}

// The stream-form launch of a family: instance(m-tiles, waves) returns the kernel instance of the route's pair (integral constants, as
// in with_stream_form); `kernel` names it in the no-instantiation error, `what` is the text a failed launch reports.
template <bool MT4_W16, typename Args, typename Instance>
int launch_stream_form(const char* kernel, const char* what, const TwoFormRoute& r, const Args& a, hipStream_t st, Instance&& instance) {
  if (int rc = with_stream_form<MT4_W16>(kernel, r, [&](auto mt, auto waves) {
        ao::launch(instance(mt, waves), dim3(r.grid_x, r.grid_y), dim3(64 * decltype(waves)::value), 0, st, a);
      }))
    return rc;
  AO_LAUNCH_CHECK(what);
  return AO_OK;
}

// The tiled-form launch: four waves on the route's grid.  lds_bytes of dynamic LDS, opted into under the text lds_what (0: none).
template <typename Kernel, typename Args>
int launch_tile_form(Kernel kernel, const char* what, const TwoFormRoute& r, const Args& a, hipStream_t st, size_t lds_bytes = 0,
                     const char* lds_what = nullptr) {
  if (lds_bytes != 0)
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds_bytes, lds_what)) return rc;
  ao::launch(kernel, dim3(r.grid_x, r.grid_y), dim3(256), lds_bytes, st, a);
  AO_LAUNCH_CHECK(what);
  return AO_OK;
}

}  // namespace ao
