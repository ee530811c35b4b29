// view_host.cpp — vg_view_gain, host side: the argument checks, the state check
// of the device grid it may read and the drain of outstanding work (the kernels
// and their buffers: view.hip).
#include "vg_host.h"

namespace vg {

int host_view_gain(vg_ctx* ctx, const int8_t* grid, const vg_view_params* prm, const int32_t* views, int n_views,
                   vg_view_rec* recs, int32_t* seen, vg_view_summary* out) {
  if (ctx->shard.world > 1) {
    ctx->err = "vg_view_gain: the context is sharded (world > 1)";
    return VG_E_STATE;
  }
  VG_TRY(host_quiesce(ctx));
  if (!grid && (!ctx->occ.grid || ctx->occ.nx != prm->nx || ctx->occ.ny != prm->ny)) {
    ctx->err = ctx->occ.nx ? "vg_view_gain: grid == NULL, and the last vg_occupancy call's nx, ny differ from prm's"
                           : "vg_view_gain: grid == NULL, and no vg_occupancy call left a grid on this context";
    return VG_E_STATE;
  }
  return view_gain_dev(ctx, grid, prm, views, n_views, recs, seen, out);
}

}  // namespace vg

extern "C" int vg_view_gain(vg_ctx* ctx, const int8_t* grid, const vg_view_params* prm, const int32_t* views,
                            int n_views, vg_view_rec* recs, int32_t* seen, vg_view_summary* out) {
  if (!ctx || !prm || !views || !recs || !out) return VG_E_ARG;
  if (prm->nx < 1 || prm->ny < 1 || prm->nx > VG_CLR_MAX_SIDE || prm->ny > VG_CLR_MAX_SIDE ||
      (long long)prm->nx * (long long)prm->ny > (long long)VG_OCC_MAX_CELLS)
    return VG_E_ARG;
  if (prm->radius < 1 || prm->radius > VG_VIEW_MAX_RADIUS || prm->max_unknown < 0 || prm->flags != 0) return VG_E_ARG;
  if (n_views < 1 || n_views > VG_NAV_MAX_POINTS) return VG_E_ARG;
  return vg::host_view_gain(ctx, grid, prm, views, n_views, recs, seen, out);
}
