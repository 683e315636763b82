// Host only: the route of a linear family that has a weight-streaming form and an LDS-tiled form -- the MX dense linears
// (mx_linear_kernels.hip) and the int8 / float8 weight-only linears (wo8_kernels.hip).  A family keeps what it measured or what its
// kernels need: its shape check, the row counts at which it hands over from the stream form to the tiled form, the tile edge of its
// tiled form and its own thread-local forced form (ao_*_linear_set_form).  The plan of either form, the grid-row cap, the fields
// ao_*_linear_route report and the compile-time (m-tiles, waves) pair of a stream-form launch are here, once.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "common.h"

namespace ao {

// ao_mx_linear_route and ao_wo8_linear_route write these seven fields, in this order (write_route)
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

}  // namespace ao
