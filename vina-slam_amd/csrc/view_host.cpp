// view_host.cpp — vg_view_gain, host side: the argument checks, the state check
// of the device grid it may read and the drain of outstanding work (the kernels
// and their buffers: view.hip).
#include "vg_host.h"
#include "vg_query.h"

namespace vg {

int host_view_gain(vg_ctx* ctx, const int8_t* grid, const vg_view_params* prm, const int32_t* views, int n_views,
                   vg_view_rec* recs, int32_t* seen, vg_view_summary* out) {
  VG_TRY(query_open(ctx, "vg_view_gain"));
  if (!grid) VG_TRY(held_grid_ok(ctx, "vg_view_gain", "grid == NULL", prm->nx, prm->ny));
  return view_gain_dev(ctx, grid, prm, views, n_views, recs, seen, out);
}

}  // namespace vg

extern "C" int vg_view_gain(vg_ctx* ctx, const int8_t* grid, const vg_view_params* prm, const int32_t* views,
                            int n_views, vg_view_rec* recs, int32_t* seen, vg_view_summary* out) {
  if (!ctx || !prm || !views || !recs || !out) return VG_E_ARG;
  if (!vg::grid_shape_ok(prm->nx, prm->ny, VG_CLR_MAX_SIDE)) return VG_E_ARG;
  if (prm->radius < 1 || prm->radius > VG_VIEW_MAX_RADIUS || prm->max_unknown < 0 || prm->flags != 0) return VG_E_ARG;
  if (n_views < 1 || n_views > VG_NAV_MAX_POINTS) return VG_E_ARG;
  return vg::host_view_gain(ctx, grid, prm, views, n_views, recs, seen, out);
}
