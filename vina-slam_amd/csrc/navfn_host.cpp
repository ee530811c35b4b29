// navfn_host.cpp — vg_navfn and vg_nav_paths, host side: the argument checks, the
// default traversal table and the drain of outstanding work (the kernels and
// their buffers: navfn.hip).
#include <cmath>

#include "vg_host.h"

namespace vg {

// vina_gpu.h's default table of prm (zeros: nav2's values); false where an entry overflows uint16
static bool nav_table(const vg_nav_params* p, uint16_t* trav) {
  const int neutral = p->neutral ? p->neutral : 50, lethal_from = p->lethal_from ? p->lethal_from : 253;
  const double factor = p->factor != 0.0 ? p->factor : 0.8;
  for (int c = 0; c < 256; c++) {
    double v = 0.0;
    if (c < lethal_from && c < 255) v = (double)neutral + std::floor(factor * (double)c);
    if (!(v <= 65535.0)) return false;
    trav[c] = (uint16_t)v;
  }
  if (p->flags & 1) trav[255] = trav[p->unknown_as];
  return true;
}

int host_navfn(vg_ctx* ctx, const uint8_t* cost, const vg_nav_params* prm, const uint16_t* trav, const int32_t* goals,
               int n_goals, uint32_t* pot, vg_nav_summary* out) {
  uint16_t table[256];
  if (trav) memcpy(table, trav, sizeof(table));
  else if (!nav_table(prm, table)) return VG_E_ARG;
  if (ctx->shard.world > 1) {
    ctx->err = "vg_navfn: the context is sharded (world > 1)";
    return VG_E_STATE;
  }
  VG_TRY(host_quiesce(ctx));
  if (!cost && (!ctx->clr.cost || ctx->clr.nx != prm->nx || ctx->clr.ny != prm->ny)) {
    ctx->err = ctx->clr.nx ? "vg_navfn: cost == NULL, and the last vg_clearance call's nx, ny differ from prm's"
                           : "vg_navfn: cost == NULL, and no vg_clearance call left a cost plane on this context";
    return VG_E_STATE;
  }
  return navfn_dev(ctx, cost, prm, table, goals, n_goals, pot, out);
}

int host_nav_paths(vg_ctx* ctx, const int32_t* starts, int n_starts, int max_len, int32_t* cells, int32_t* len,
                   int32_t* status, int64_t* path_cost) {
  if (ctx->shard.world > 1) {
    ctx->err = "vg_nav_paths: the context is sharded (world > 1)";
    return VG_E_STATE;
  }
  VG_TRY(host_quiesce(ctx));
  if (!ctx->nav.nx) {
    ctx->err = "vg_nav_paths: no vg_navfn call left a field on this context";
    return VG_E_STATE;
  }
  return nav_paths_dev(ctx, starts, n_starts, max_len, cells, len, status, path_cost);
}

}  // namespace vg

extern "C" int vg_navfn(vg_ctx* ctx, const uint8_t* cost, const vg_nav_params* prm, const uint16_t* trav,
                        const int32_t* goals, int n_goals, uint32_t* pot, vg_nav_summary* out) {
  if (!ctx || !prm || !goals || !out) return VG_E_ARG;
  if (prm->nx < 1 || prm->ny < 1 || prm->nx > VG_CLR_MAX_SIDE || prm->ny > VG_CLR_MAX_SIDE ||
      (long long)prm->nx * (long long)prm->ny > (long long)VG_OCC_MAX_CELLS)
    return VG_E_ARG;
  if (n_goals < 1 || n_goals > VG_NAV_MAX_POINTS) return VG_E_ARG;
  if (prm->flags & ~1) return VG_E_ARG;
  if (prm->neutral < 0 || prm->lethal_from < 0 || prm->lethal_from > 255 || prm->unknown_as < 0 || prm->unknown_as > 254)
    return VG_E_ARG;
  if (!(prm->factor >= 0.0) || !std::isfinite(prm->factor)) return VG_E_ARG;
  return vg::host_navfn(ctx, cost, prm, trav, goals, n_goals, pot, out);
}

extern "C" int vg_nav_paths(vg_ctx* ctx, const int32_t* starts, int n_starts, int max_len, int32_t* cells, int32_t* len,
                            int32_t* status, int64_t* path_cost) {
  if (!ctx || !starts || !cells || !len || !status) return VG_E_ARG;
  if (n_starts < 1 || n_starts > VG_NAV_MAX_POINTS || max_len < 1 ||
      (long long)n_starts * (long long)max_len > (long long)VG_NAV_MAX_PATH_CELLS)
    return VG_E_ARG;
  return vg::host_nav_paths(ctx, starts, n_starts, max_len, cells, len, status, path_cost);
}
