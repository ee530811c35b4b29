// navfn_host.cpp — vg_navfn and vg_nav_paths, host side: the argument checks, the
// default traversal table and the drain of outstanding work (the kernels and
// their buffers: navfn.hip).
#include <cmath>

#include "vg_host.h"
#include "vg_query.h"

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
  VG_TRY(query_open(ctx, "vg_navfn"));
  if (!cost) VG_TRY(held_cost_ok(ctx, "vg_navfn", "cost == NULL", prm->nx, prm->ny));
  return navfn_dev(ctx, cost, prm, table, goals, n_goals, pot, out);
}

int host_nav_paths(vg_ctx* ctx, const int32_t* starts, int n_starts, int max_len, int32_t* cells, int32_t* len,
                   int32_t* status, int64_t* path_cost) {
  VG_TRY(query_open(ctx, "vg_nav_paths"));
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
  if (!vg::grid_shape_ok(prm->nx, prm->ny, VG_CLR_MAX_SIDE)) return VG_E_ARG;
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
