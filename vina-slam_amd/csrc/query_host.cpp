// query_host.cpp — the opening and the state checks the query layers' host_*
// functions share (vg_query.h).
#include "vg_query.h"

namespace vg {

int query_open(vg_ctx* ctx, const char* who) {
  if (ctx->shard.world > 1) {
    ctx->err = std::string(who) + ": the context is sharded (world > 1)";
    return VG_E_STATE;
  }
  return host_quiesce(ctx);
}

// held: the plane exists; hx, hy: its shape (0: no call has left one); by: the call that leaves it
static int held_ok(vg_ctx* ctx, const char* who, const char* what, bool held, int hx, int hy, int nx, int ny,
                   const char* by, const char* plane) {
  if (held && hx == nx && hy == ny) return VG_OK;
  ctx->err = std::string(who) + ": " + what +
             (hx ? std::string(", and the last ") + by + " call's nx, ny differ from prm's"
                 : std::string(", and no ") + by + " call left " + plane + " on this context");
  return VG_E_STATE;
}

int held_grid_ok(vg_ctx* ctx, const char* who, const char* what, int nx, int ny) {
  return held_ok(ctx, who, what, ctx->occ.grid.p != nullptr, ctx->occ.nx, ctx->occ.ny, nx, ny, "vg_occupancy", "a grid");
}
int held_cost_ok(vg_ctx* ctx, const char* who, const char* what, int nx, int ny) {
  return held_ok(ctx, who, what, ctx->clr.cost.p != nullptr, ctx->clr.nx, ctx->clr.ny, nx, ny, "vg_clearance",
                 "a cost plane");
}
int held_field_ok(vg_ctx* ctx, const char* who, const char* what, int nx, int ny) {
  return held_ok(ctx, who, what, true, ctx->nav.nx, ctx->nav.ny, nx, ny, "vg_navfn", "a field");
}

}  // namespace vg
