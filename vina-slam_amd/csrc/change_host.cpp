// change_host.cpp — the change layer behind the C-ABI (vina_gpu.h "Change
// layer"): the state checks, the drain of outstanding work, the mutex that
// serialises the calls into one layer, and the totals kept on the host (the
// kernels and the layer's memory: change.hip).
#include <algorithm>
#include <cstring>

#include "vg_host.h"

namespace vg {

static vg_ctx* map_owner(vg_ctx* ctx) { return ctx->view_of ? ctx->view_of : ctx; }

static int state_err(vg_ctx* ctx, const char* who, const char* why) {
  ctx->err = std::string(who) + ": " + why;
  return VG_E_STATE;
}

int host_change_begin(vg_ctx* ctx, const vg_change_params* prm) {
  const char* who = "vg_change_begin";
  std::lock_guard<std::mutex> lock(ctx->change_mu);
  if (ctx->mapping) return state_err(ctx, who, "mapping is on (vg_set_mapping(ctx, 0) first)");
  if (sharded(ctx) || ctx->shard.world > 1) return state_err(ctx, who, "the context is sharded");
  if (hp(ctx)->in_scan) return state_err(ctx, who, "the context is inside a scan (vg_step_end first)");
  if (ctx->view_of) return state_err(ctx, who, "the context is attached to another context's map (begin on the owner)");
  if (ctx->change) return state_err(ctx, who, "the context has a change layer already (vg_change_end first)");
  const int log2 = prm && prm->cell_hash_log2 > 0 ? prm->cell_hash_log2 : 20;
  if (log2 > 26) {
    ctx->err = std::string(who) + ": cell_hash_log2 above 26";
    return VG_E_ARG;
  }
  VG_TRY(host_quiesce(ctx));
  ChangeLayer* L = new ChangeLayer();
  memset(&L->diff, 0, sizeof(L->diff));
  if (prm) L->diff = prm->diff;
  L->d.cell_size = prm && prm->cell > 0.0 ? prm->cell : hp(ctx)->mpd.vs / 4.0;
  int r = change_alloc(ctx, L, log2);
  if (r == VG_OK) r = change_clear_dev(ctx, L);
  if (r != VG_OK) {
    delete L;
    return r;
  }
  ctx->change = L;
  return VG_OK;
}

// xyz != nullptr: the host cloud; else the three device arrays
int host_change_accumulate(vg_ctx* ctx, const float* xyz, const float* d_x, const float* d_y, const float* d_z, int n,
                           const double* pose12, vg_diff_point* per_point, vg_diff_summary* out) {
  const char* who = "vg_change_accumulate";
  if (ctx->shard.world > 1) return state_err(ctx, who, "the context is sharded (world > 1)");
  VG_TRY(host_quiesce(ctx));
  double pose[12];
  if (pose12) {
    memcpy(pose, pose12, sizeof(pose));
  } else {  // the calling context's current state (the host mirror, current after the drain)
    const HX& x = hp(ctx)->x_curr;
    memcpy(pose, x.R.a, 72);
    memcpy(pose + 9, x.p.a, 24);
  }
  vg_diff_summary sum;
  vg_ctx* owner = map_owner(ctx);
  std::lock_guard<std::mutex> lock(owner->change_mu);
  ChangeLayer* L = owner->change;  // read under the lock: vg_change_end on another thread cannot free it under this call
  if (!L) return state_err(ctx, who, "the map this context reads has no change layer (vg_change_begin on its owner)");
  const int epoch = L->epoch + 1;  // taken for good only when the call succeeds
  int r;
  if (xyz) r = change_accum_dev(ctx, L, hp(ctx)->mpd, xyz, nullptr, nullptr, 3, false, n, pose, epoch, per_point, &sum);
  else r = change_accum_dev(ctx, L, hp(ctx)->mpd, d_x, d_y, d_z, 1, true, n, pose, epoch, nullptr, &sum);
  if (r != VG_OK) return r;
  L->epoch = epoch;
  L->calls++;
  L->points += n;
  for (int c = 0; c < 4; c++) L->cls[c] += sum.n[c];
  if (out) *out = sum;
  return VG_OK;
}

int host_change_report(vg_ctx* ctx, const vg_change_query* q, vg_change_leaf* leaves, int leaf_cap, int* n_leaves,
                       vg_change_cell* cells, int cell_cap, int* n_cells, vg_change_totals* totals) {
  VG_TRY(host_quiesce(ctx));
  vg_change_query query;
  memset(&query, 0, sizeof(query));
  if (q) query = *q;
  std::vector<vg_change_leaf> lv;
  std::vector<vg_change_cell> cv;
  long long tot4[4] = {0, 0, 0, 0};
  vg_ctx* owner = map_owner(ctx);
  std::lock_guard<std::mutex> lock(owner->change_mu);
  ChangeLayer* L = owner->change;
  if (!L) return state_err(ctx, "vg_change_report", "the map this context reads has no change layer");
  VG_TRY(change_report_dev(ctx, L, query, lv, cv, tot4));
  if (n_leaves) *n_leaves = (int)lv.size();
  if (n_cells) *n_cells = (int)cv.size();
  if (leaves && leaf_cap > 0 && !lv.empty())
    memcpy(leaves, lv.data(), std::min((size_t)leaf_cap, lv.size()) * sizeof(vg_change_leaf));
  if (cells && cell_cap > 0 && !cv.empty())
    memcpy(cells, cv.data(), std::min((size_t)cell_cap, cv.size()) * sizeof(vg_change_cell));
  if (totals) {
    memset(totals, 0, sizeof(*totals));
    totals->calls = L->calls;
    totals->points = L->points;
    for (int c = 0; c < 4; c++) totals->n[c] = L->cls[c];
    totals->dropped = tot4[0];
    totals->out_of_range = tot4[1];
    totals->leaves_touched = tot4[2];
    totals->cells_used = tot4[3];
  }
  return VG_OK;
}

// the caller holds ctx->change_mu
static int owner_layer(vg_ctx* ctx, const char* who, ChangeLayer** L) {
  if (ctx->view_of) return state_err(ctx, who, "the context is attached: the layer belongs to the map's owner");
  if (!ctx->change) return state_err(ctx, who, "the context has no change layer");
  *L = ctx->change;
  return VG_OK;
}

int host_change_clear(vg_ctx* ctx) {
  ChangeLayer* L = nullptr;
  VG_TRY(host_quiesce(ctx));
  std::lock_guard<std::mutex> lock(ctx->change_mu);
  VG_TRY(owner_layer(ctx, "vg_change_clear", &L));
  VG_TRY(change_clear_dev(ctx, L));
  L->epoch = 0;
  L->calls = L->points = 0;
  for (int c = 0; c < 4; c++) L->cls[c] = 0;
  return VG_OK;
}

int host_change_end(vg_ctx* ctx) {
  ChangeLayer* L = nullptr;
  // a call in flight on another thread finishes first; one that waits for the lock finds no layer (VG_E_STATE)
  std::lock_guard<std::mutex> lock(ctx->change_mu);
  VG_TRY(owner_layer(ctx, "vg_change_end", &L));
  ctx->change = nullptr;
  delete L;
  return VG_OK;
}

}  // namespace vg

extern "C" {
int vg_change_begin(vg_ctx* ctx, const vg_change_params* prm) {
  if (!ctx) return VG_E_ARG;
  return vg::host_change_begin(ctx, prm);
}
int vg_change_accumulate(vg_ctx* ctx, const float* xyz, int n, const double* pose12, vg_diff_point* per_point,
                         vg_diff_summary* out) {
  if (!ctx || n < 0 || (n > 0 && !xyz) || n > ctx->cap.max_points_per_scan) return VG_E_ARG;
  static const float none[3] = {0, 0, 0};
  return vg::host_change_accumulate(ctx, n > 0 ? xyz : none, nullptr, nullptr, nullptr, n, pose12, per_point, out);
}
int vg_change_accumulate_dev(vg_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int n,
                             const double* pose12, vg_diff_summary* out) {
  if (!ctx || n < 0 || (n > 0 && (!d_x || !d_y || !d_z)) || n > ctx->cap.max_points_per_scan) return VG_E_ARG;
  return vg::host_change_accumulate(ctx, nullptr, d_x, d_y, d_z, n, pose12, nullptr, out);
}
int vg_change_report(vg_ctx* ctx, const vg_change_query* q, vg_change_leaf* leaves, int leaf_cap, int* n_leaves,
                     vg_change_cell* cells, int cell_cap, int* n_cells, vg_change_totals* totals) {
  if (!ctx || leaf_cap < 0 || cell_cap < 0) return VG_E_ARG;
  return vg::host_change_report(ctx, q, leaves, leaf_cap, n_leaves, cells, cell_cap, n_cells, totals);
}
int vg_change_clear(vg_ctx* ctx) {
  if (!ctx) return VG_E_ARG;
  return vg::host_change_clear(ctx);
}
int vg_change_end(vg_ctx* ctx) {
  if (!ctx) return VG_E_ARG;
  return vg::host_change_end(ctx);
}
}
