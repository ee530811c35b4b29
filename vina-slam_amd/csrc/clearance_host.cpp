// clearance_host.cpp — vg_clearance, host side: the argument checks, the cost
// table and the drain of outstanding work (the kernels and their buffers:
// clearance.hip).
#include <cmath>
#include <vector>

#include "vg_host.h"
#include "vg_query.h"

namespace vg {

// vina_gpu.h's cost of a cell at dist2 cells squared from the nearest obstacle, in double
static uint8_t clr_cost(const vg_clr_params* p, long long dist2) {
  if (dist2 == 0) return VG_COST_LETHAL;
  const double d = p->res * std::sqrt((double)dist2);
  if (d <= p->inscribed_radius) return VG_COST_INSCRIBED;
  if (d <= p->inflation_radius) return (uint8_t)(252.0 * std::exp(-p->cost_scaling * (d - p->inscribed_radius)));
  return VG_COST_FREE;
}

int host_clearance(vg_ctx* ctx, const int8_t* grid, const vg_clr_params* prm, int32_t* dist2, int32_t* nearest,
                   uint8_t* cost, vg_clr_summary* out) {
  VG_TRY(query_open(ctx, "vg_clearance"));
  // entries 0 .. floor((inflation_radius / res)^2), and one more evaluated the same way, so that a dist2 whose d
  // rounds onto the radius is still looked up; past it the cost is 0. No entry beyond the grid's largest dist2
  const double q = (prm->inflation_radius / prm->res) * (prm->inflation_radius / prm->res);
  const long long far = (long long)(prm->nx - 1) * (prm->nx - 1) + (long long)(prm->ny - 1) * (prm->ny - 1);
  const long long want = (long long)std::floor(q) + 2;
  const int table_n = (int)(want < far + 1 ? want : far + 1);
  if (!grid) VG_TRY(held_grid_ok(ctx, "vg_clearance", "grid == NULL", prm->nx, prm->ny));
  std::vector<uint8_t> table;
  if (!clr_table_current(ctx, prm, table_n)) {
    table.resize((size_t)table_n);
    for (int i = 0; i < table_n; i++) table[i] = clr_cost(prm, i);
  }
  return clearance_dev(ctx, grid, prm, table.empty() ? nullptr : table.data(), table_n, dist2, nearest, cost, out);
}

}  // namespace vg

extern "C" int vg_clearance(vg_ctx* ctx, const int8_t* grid, const vg_clr_params* prm, int32_t* dist2,
                            int32_t* nearest, uint8_t* cost, vg_clr_summary* out) {
  if (!ctx || !prm || !out) return VG_E_ARG;
  if (!vg::grid_shape_ok(prm->nx, prm->ny, VG_CLR_MAX_SIDE)) return VG_E_ARG;
  if (!(prm->res > 0.0) || !std::isfinite(prm->res)) return VG_E_ARG;
  if (!(prm->inscribed_radius >= 0.0) || !std::isfinite(prm->inscribed_radius) || !std::isfinite(prm->inflation_radius) ||
      !(prm->inflation_radius >= prm->inscribed_radius) || !(prm->cost_scaling >= 0.0) || !std::isfinite(prm->cost_scaling))
    return VG_E_ARG;
  if (prm->flags & ~1) return VG_E_ARG;
  const double q = (prm->inflation_radius / prm->res) * (prm->inflation_radius / prm->res);
  if (!(q < (double)(1 << 24))) return VG_E_ARG;  // (a table of floor(q) + 1 entries; an overflow to inf too)
  return vg::host_clearance(ctx, grid, prm, dist2, nearest, cost, out);
}
