// frontier_host.cpp — vg_frontiers, host side: the argument checks, the state
// checks of the three device planes it may read and the drain of outstanding
// work (the kernels and their buffers: frontier.hip).
#include "vg_host.h"

namespace vg {

int host_frontiers(vg_ctx* ctx, const int8_t* grid, const uint8_t* cost, const vg_frontier_params* prm, int32_t* labels,
                   vg_frontier_rec* recs, int max_records, vg_frontier_summary* out) {
  if (ctx->shard.world > 1) {
    ctx->err = "vg_frontiers: the context is sharded (world > 1)";
    return VG_E_STATE;
  }
  VG_TRY(host_quiesce(ctx));
  if (!grid && (!ctx->occ.grid || ctx->occ.nx != prm->nx || ctx->occ.ny != prm->ny)) {
    ctx->err = ctx->occ.nx ? "vg_frontiers: grid == NULL, and the last vg_occupancy call's nx, ny differ from prm's"
                           : "vg_frontiers: grid == NULL, and no vg_occupancy call left a grid on this context";
    return VG_E_STATE;
  }
  if ((prm->flags & 1) && !cost && (!ctx->clr.cost || ctx->clr.nx != prm->nx || ctx->clr.ny != prm->ny)) {
    ctx->err = ctx->clr.nx ? "vg_frontiers: cost == NULL, and the last vg_clearance call's nx, ny differ from prm's"
                           : "vg_frontiers: cost == NULL, and no vg_clearance call left a cost plane on this context";
    return VG_E_STATE;
  }
  if ((prm->flags & 2) && (ctx->nav.nx != prm->nx || ctx->nav.ny != prm->ny)) {
    ctx->err = ctx->nav.nx ? "vg_frontiers: flags bit 1, and the last vg_navfn call's nx, ny differ from prm's"
                           : "vg_frontiers: flags bit 1, and no vg_navfn call left a field on this context";
    return VG_E_STATE;
  }
  return frontiers_dev(ctx, grid, cost, prm, labels, recs, max_records, out);
}

}  // namespace vg

extern "C" int vg_frontiers(vg_ctx* ctx, const int8_t* grid, const uint8_t* cost, const vg_frontier_params* prm,
                            int32_t* labels, vg_frontier_rec* recs, int max_records, vg_frontier_summary* out) {
  if (!ctx || !prm || !out) return VG_E_ARG;
  if (prm->nx < 1 || prm->ny < 1 || prm->nx > VG_CLR_MAX_SIDE || prm->ny > VG_CLR_MAX_SIDE ||
      (long long)prm->nx * (long long)prm->ny > (long long)VG_OCC_MAX_CELLS)
    return VG_E_ARG;
  if (prm->flags & ~3) return VG_E_ARG;
  if (cost && !(prm->flags & 1)) return VG_E_ARG;
  if (prm->cost_max < 0 || prm->cost_max > 255) return VG_E_ARG;
  if (max_records < 0 || max_records > VG_FRONTIER_MAX_RECORDS || (!recs && max_records > 0)) return VG_E_ARG;
  return vg::host_frontiers(ctx, grid, cost, prm, labels, recs, max_records, out);
}
