// occupancy_host.cpp — vg_occupancy, host side: the argument checks and the
// drain of outstanding work (the kernels and their buffers: occupancy.hip).
#include <cmath>

#include "vg_host.h"

namespace vg {

int host_occupancy(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D, const vg_occ_params* prm,
                   int8_t* grid, int32_t* counts, vg_occ_summary* out) {
  if (ctx->shard.world > 1) {
    ctx->err = "vg_occupancy: the context is sharded (world > 1)";
    return VG_E_STATE;
  }
  VG_TRY(host_quiesce(ctx));
  return occupancy_dev(ctx, hp(ctx)->mpd, positions, M, dirs, D, prm, grid, counts, out);
}

}  // namespace vg

extern "C" int vg_occupancy(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D,
                            const vg_occ_params* prm, int8_t* grid, int32_t* counts, vg_occ_summary* out) {
  if (!ctx || !prm || !grid || !out || !dirs || M < 0 || (M > 0 && !positions)) return VG_E_ARG;
  if (D < 1 || D > vg::kInfoMaxDirs) return VG_E_ARG;
  if (!(prm->res > 0.0) || !std::isfinite(prm->res) || !std::isfinite(prm->x0) || !std::isfinite(prm->y0))
    return VG_E_ARG;
  if (prm->nx < 1 || prm->ny < 1 || (long long)prm->nx * (long long)prm->ny > (long long)VG_OCC_MAX_CELLS)
    return VG_E_ARG;
  if (!(prm->z_lo < prm->z_hi) || (prm->flags & ~1)) return VG_E_ARG;
  return vg::host_occupancy(ctx, positions, M, dirs, D, prm, grid, counts, out);
}
