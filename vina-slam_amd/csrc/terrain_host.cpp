// terrain_host.cpp — vg_terrain, host side: the argument checks and the drain
// of outstanding work (the kernels, their buffers and the defaults: terrain.hip,
// vg_terrain.h).
#include <cmath>

#include "vg_host.h"
#include "vg_query.h"

namespace vg {

int host_terrain(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D, const vg_terrain_params* prm,
                 int8_t* grid, int32_t* elev, int32_t* step, int32_t* counts, vg_terrain_summary* out) {
  VG_TRY(query_open(ctx, "vg_terrain"));
  return terrain_dev(ctx, hp(ctx)->mpd, positions, M, dirs, D, prm, grid, elev, step, counts, out);
}

// both 0 (the defaults), or lo < hi
static bool ter_pair_ok(double lo, double hi) { return (lo == 0.0 && hi == 0.0) || lo < hi; }

}  // namespace vg

extern "C" int vg_terrain(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D,
                          const vg_terrain_params* prm, int8_t* grid, int32_t* elev, int32_t* step, int32_t* counts,
                          vg_terrain_summary* out) {
  if (!vg::ray_grid_args_ok(ctx, positions, M, dirs, D, prm, grid, out)) return VG_E_ARG;
  if (prm->flags & ~3) return VG_E_ARG;
  if (!std::isfinite(prm->z_res) || !std::isfinite(prm->up_min)) return VG_E_ARG;
  if (!vg::ter_pair_ok(prm->g_lo, prm->g_hi) || !vg::ter_pair_ok(prm->clear_lo, prm->clear_hi)) return VG_E_ARG;
  if (!std::isfinite(prm->sensor_height) || prm->sensor_height < 0.0) return VG_E_ARG;
  if ((prm->flags & 2) && (!std::isfinite(prm->step_max) || prm->step_max < 0.0)) return VG_E_ARG;
  return vg::host_terrain(ctx, positions, M, dirs, D, prm, grid, elev, step, counts, out);
}
