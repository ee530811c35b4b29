// live_host.cpp — the live obstacle layer behind the C-ABI (vina_gpu.h "Live
// obstacle layer"): the argument checks, the defaults, the state checks, the
// drain of outstanding work, the stamps and the totals kept on the host (the
// kernels and the layer's memory: live.hip).
#include <climits>
#include <cmath>
#include <cstring>

#include "vg_host.h"
#include "vg_query.h"

namespace vg {

static int state_err(vg_ctx* ctx, const char* who, const char* why) {
  ctx->err = std::string(who) + ": " + why;
  return VG_E_STATE;
}

// the opening every call but vg_live_begin shares: the query's, then the layer
static int live_open(vg_ctx* ctx, const char* who, LiveLayer** L) {
  VG_TRY(query_open(ctx, who));
  if (!ctx->live) return state_err(ctx, who, "the context has no live layer (vg_live_begin first)");
  *L = ctx->live;
  return VG_OK;
}

// prm with the defaults applied; false: an argument error
static bool live_prm(const vg_live_params* p, LivePrm* q) {
  if (!(p->res > 0.0) || !std::isfinite(p->res) || !std::isfinite(p->x0) || !std::isfinite(p->y0)) return false;
  if (!grid_shape_ok(p->nx, p->ny, VG_CLR_MAX_SIDE)) return false;
  if (p->flags & ~1) return false;
  q->x0 = p->x0, q->y0 = p->y0, q->res = p->res, q->nx = p->nx, q->ny = p->ny;
  q->z_lo = p->z_lo, q->z_hi = p->z_hi;
  if (p->z_lo == 0.0 && p->z_hi == 0.0) q->z_lo = -1.0, q->z_hi = 1.0;
  if (!std::isfinite(q->z_lo) || !std::isfinite(q->z_hi)) return false;
  if (!(q->z_lo <= 0.0 && 0.0 <= q->z_hi && q->z_lo < q->z_hi)) return false;
  q->r_min = p->r_min > 0.0 ? p->r_min : 0.0;
  q->mark_max = p->mark_max > 0.0 ? p->mark_max : HUGE_VAL;
  q->clear_max = p->clear_max > 0.0 ? p->clear_max : 4096.0 * p->res;
  if (!(p->clear_max > 0.0) && q->mark_max < q->clear_max) q->clear_max = q->mark_max;
  if (!(q->clear_max / p->res <= 4096.0)) return false;  // (a NaN fails too)
  q->persist = p->persist > 0 ? p->persist : 0;
  q->unknown_marks = p->flags & 1;
  return true;
}

int host_live_begin(vg_ctx* ctx, const vg_live_params* prm, const int8_t* base_grid) {
  const char* who = "vg_live_begin";
  LivePrm q;
  if (!live_prm(prm, &q)) return VG_E_ARG;
  VG_TRY(query_open(ctx, who));
  if (ctx->live) return state_err(ctx, who, "the context has a live layer already (vg_live_end first)");
  if (!base_grid) VG_TRY(held_grid_ok(ctx, who, "base_grid == NULL", q.nx, q.ny));
  LiveLayer* L = new LiveLayer();
  L->q = q;
  L->diff = prm->diff;
  const int r = live_alloc(ctx, L, base_grid);
  if (r != VG_OK) {
    delete L;
    return r;
  }
  ctx->live = L;
  return VG_OK;
}

// xyz != nullptr: the host cloud; else the three device arrays
int host_live_mark(vg_ctx* ctx, const float* xyz, const float* d_x, const float* d_y, const float* d_z, int n,
                   const double* pose12, int stamp, vg_live_point* per_point, vg_live_summary* out) {
  const char* who = "vg_live_mark";
  LiveLayer* L = nullptr;
  VG_TRY(live_open(ctx, who, &L));
  if (stamp == 0) {
    if (L->stamp == INT_MAX) {
      ctx->err = std::string(who) + ": stamp == 0 and the layer's largest stamp is INT32_MAX (vg_live_clear)";
      return VG_E_RANGE;
    }
    stamp = L->stamp + 1;
  }
  double pose[12];
  if (pose12) {
    memcpy(pose, pose12, sizeof(pose));
  } else {  // the context's current state (the host mirror, current after the drain)
    const HX& x = hp(ctx)->x_curr;
    memcpy(pose, x.R.a, 72);
    memcpy(pose + 9, x.p.a, 24);
  }
  vg_live_summary sum;
  if (xyz) VG_TRY(live_mark_dev(ctx, L, hp(ctx)->mpd, xyz, nullptr, nullptr, 3, false, n, pose, stamp, per_point, &sum));
  else VG_TRY(live_mark_dev(ctx, L, hp(ctx)->mpd, d_x, d_y, d_z, 1, true, n, pose, stamp, nullptr, &sum));
  // the stamp and the totals are taken only once the call succeeded
  if (stamp > L->stamp) L->stamp = stamp;
  vg_live_summary& t = L->tot;
  for (int c = 0; c < 4; c++) t.n[c] += sum.n[c];
  t.n_obstacle += sum.n_obstacle, t.marks_dropped += sum.marks_dropped, t.n_beams += sum.n_beams;
  t.cells_live += sum.cells_live, t.cells_cleared += sum.cells_cleared;
  t.calls++;
  if (out) *out = sum;
  return VG_OK;
}

int host_live_compose(vg_ctx* ctx, int now, int flags, int8_t* grid, vg_live_summary* out) {
  LiveLayer* L = nullptr;
  VG_TRY(live_open(ctx, "vg_live_compose", &L));
  return live_compose_dev(ctx, L, now > 0 ? now : L->stamp, flags, grid, out);
}

int host_live_info(vg_ctx* ctx, int32_t* hit, int32_t* clear, vg_live_summary* totals) {
  LiveLayer* L = nullptr;
  VG_TRY(live_open(ctx, "vg_live_info", &L));
  const size_t bytes = (size_t)L->q.nx * (size_t)L->q.ny * sizeof(int32_t);
  hipStream_t s = ctx->stream;
  if (hit) VG_HIP(hipMemcpyAsync(hit, L->hit, bytes, hipMemcpyDeviceToHost, s));
  if (clear) VG_HIP(hipMemcpyAsync(clear, L->clear, bytes, hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  if (totals) {
    *totals = L->tot;
    totals->stamp = L->stamp;
  }
  return VG_OK;
}

int host_live_clear(vg_ctx* ctx) {
  LiveLayer* L = nullptr;
  VG_TRY(live_open(ctx, "vg_live_clear", &L));
  VG_TRY(live_clear_dev(ctx, L));
  L->stamp = 0;
  memset(&L->tot, 0, sizeof(L->tot));
  return VG_OK;
}

int host_live_end(vg_ctx* ctx) {
  LiveLayer* L = ctx->live;  // (no opening: vg_destroy ends the layer of a context in any state)
  if (!L) return state_err(ctx, "vg_live_end", "the context has no live layer");
  VG_TRY(host_quiesce(ctx));
  ctx->live = nullptr;
  delete L;
  return VG_OK;
}

}  // namespace vg

extern "C" {
int vg_live_begin(vg_ctx* ctx, const vg_live_params* prm, const int8_t* base_grid) {
  if (!ctx || !prm) return VG_E_ARG;
  return vg::host_live_begin(ctx, prm, base_grid);
}
int vg_live_mark(vg_ctx* ctx, const float* xyz, int n, const double* pose12, int32_t stamp, vg_live_point* per_point,
                 vg_live_summary* out) {
  if (!ctx || n < 0 || (n > 0 && !xyz) || n > ctx->cap.max_points_per_scan || stamp < 0) return VG_E_ARG;
  static const float none[3] = {0, 0, 0};
  return vg::host_live_mark(ctx, n > 0 ? xyz : none, nullptr, nullptr, nullptr, n, pose12, stamp, per_point, out);
}
int vg_live_mark_dev(vg_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int n, const double* pose12,
                     int32_t stamp, vg_live_summary* out) {
  if (!ctx || n < 0 || (n > 0 && (!d_x || !d_y || !d_z)) || n > ctx->cap.max_points_per_scan || stamp < 0)
    return VG_E_ARG;
  return vg::host_live_mark(ctx, nullptr, d_x, d_y, d_z, n, pose12, stamp, nullptr, out);
}
int vg_live_compose(vg_ctx* ctx, int32_t now, int flags, int8_t* grid, vg_live_summary* out) {
  if (!ctx || now < 0 || (flags & ~1)) return VG_E_ARG;
  return vg::host_live_compose(ctx, now, flags, grid, out);
}
int vg_live_info(vg_ctx* ctx, int32_t* hit, int32_t* clear, vg_live_summary* totals) {
  if (!ctx) return VG_E_ARG;
  return vg::host_live_info(ctx, hit, clear, totals);
}
int vg_live_clear(vg_ctx* ctx) {
  if (!ctx) return VG_E_ARG;
  return vg::host_live_clear(ctx);
}
int vg_live_end(vg_ctx* ctx) {
  if (!ctx) return VG_E_ARG;
  return vg::host_live_end(ctx);
}
}
