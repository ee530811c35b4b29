// frontier_host.cpp — vg_frontiers, host side: the argument checks, the state
// checks of the three device planes it may read and the drain of outstanding
// work (the kernels and their buffers: frontier.hip).
#include "vg_host.h"
#include "vg_query.h"

namespace vg {

int host_frontiers(vg_ctx* ctx, const int8_t* grid, const uint8_t* cost, const vg_frontier_params* prm, int32_t* labels,
                   vg_frontier_rec* recs, int max_records, vg_frontier_summary* out) {
  VG_TRY(query_open(ctx, "vg_frontiers"));
  if (!grid) VG_TRY(held_grid_ok(ctx, "vg_frontiers", "grid == NULL", prm->nx, prm->ny));
  if ((prm->flags & 1) && !cost) VG_TRY(held_cost_ok(ctx, "vg_frontiers", "cost == NULL", prm->nx, prm->ny));
  if (prm->flags & 2) VG_TRY(held_field_ok(ctx, "vg_frontiers", "flags bit 1", prm->nx, prm->ny));
  return frontiers_dev(ctx, grid, cost, prm, labels, recs, max_records, out);
}

}  // namespace vg

extern "C" int vg_frontiers(vg_ctx* ctx, const int8_t* grid, const uint8_t* cost, const vg_frontier_params* prm,
                            int32_t* labels, vg_frontier_rec* recs, int max_records, vg_frontier_summary* out) {
  if (!ctx || !prm || !out) return VG_E_ARG;
  if (!vg::grid_shape_ok(prm->nx, prm->ny, VG_CLR_MAX_SIDE)) return VG_E_ARG;
  if (prm->flags & ~3) return VG_E_ARG;
  if (cost && !(prm->flags & 1)) return VG_E_ARG;
  if (prm->cost_max < 0 || prm->cost_max > 255) return VG_E_ARG;
  if (max_records < 0 || max_records > VG_FRONTIER_MAX_RECORDS || (!recs && max_records > 0)) return VG_E_ARG;
  return vg::host_frontiers(ctx, grid, cost, prm, labels, recs, max_records, out);
}
