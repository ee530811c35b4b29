// occupancy_host.cpp — vg_occupancy, host side: the argument checks and the
// drain of outstanding work (the kernels and their buffers: occupancy.hip).
#include "vg_host.h"
#include "vg_query.h"

namespace vg {

int host_occupancy(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D, const vg_occ_params* prm,
                   int8_t* grid, int32_t* counts, vg_occ_summary* out) {
  VG_TRY(query_open(ctx, "vg_occupancy"));
  return occupancy_dev(ctx, hp(ctx)->mpd, positions, M, dirs, D, prm, grid, counts, out);
}

}  // namespace vg

extern "C" int vg_occupancy(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D,
                            const vg_occ_params* prm, int8_t* grid, int32_t* counts, vg_occ_summary* out) {
  if (!vg::ray_grid_args_ok(ctx, positions, M, dirs, D, prm, grid, out)) return VG_E_ARG;
  if (!(prm->z_lo < prm->z_hi) || (prm->flags & ~1)) return VG_E_ARG;
  return vg::host_occupancy(ctx, positions, M, dirs, D, prm, grid, counts, out);
}
