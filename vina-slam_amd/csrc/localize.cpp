// localize.cpp — localising in a saved map, host side: the frozen-map switch
// (vg_set_mapping; the frozen scan itself is pipeline.cpp frozen_step), pose
// scoring (vg_score_poses over score.hip) and relocalisation (vg_relocalize:
// the hypothesis grid, the ranking, and the LiDAR-only Gauss-Newton whose
// 6 x 6 normal equations come from the device, one launch per iteration).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "vg_host.h"

namespace vg {

// Between scans only; completes everything outstanding, so the last mapping
// scan's margi tail (and whatever device flag it publishes) is done before the
// first frozen scan is enqueued, and no hand-off of the split IEKF is left armed
int host_set_mapping(vg_ctx* ctx, int on) {
  if (on) {  // a map other contexts read, or another context's map, stays read-only
    VG_TRY(refuse_attached(ctx, "vg_set_mapping"));
    VG_TRY(refuse_owner(ctx, "vg_set_mapping"));
    VG_TRY(refuse_layer(ctx, "vg_set_mapping"));
  }
  VG_TRY(host_ckpt_allowed(ctx, "vg_set_mapping", true));  // open scan, cold start initialising, sharded world > 1
  VG_TRY(host_sync(ctx));
  if (ctx->stream_ds && ctx->stream_ds != ctx->stream) VG_HIP(hipStreamSynchronize(ctx->stream_ds));
  if (ctx->stream_iekf) VG_HIP(hipStreamSynchronize(ctx->stream_iekf));
  ctx->tail_a_valid = false;
  ctx->sync_tail_armed = false;
  ctx->mapping = on != 0;
  return VG_OK;
}

// ---- map views (vina_gpu.h "Map views"): a tracker reads the owner's frozen map
static int drain_all(vg_ctx* ctx) {
  VG_TRY(host_sync(ctx));
  if (ctx->stream_ds && ctx->stream_ds != ctx->stream) VG_HIP(hipStreamSynchronize(ctx->stream_ds));
  if (ctx->stream_iekf) VG_HIP(hipStreamSynchronize(ctx->stream_iekf));
  return VG_OK;
}

// After the attach the tracker is what a context that loaded the owner's
// checkpoint and froze it would be, without the file and without the map's
// copy: the load's own steps (checkpoint.hip checkpoint_load) on the owner's
// memory — vg_reset, DState's semantic fields (the checkpoint's list), the host
// mirror through its blob (ckpt_host.cpp) — and then the owner's DevMap in
// place of the tracker's own, which waits in own_map
int host_map_attach(vg_ctx* ctx, vg_ctx* owner) {
  const char* who = "vg_map_attach";
  auto refuse = [&](const char* why, int code) {
    ctx->err = std::string(who) + ": " + why;
    owner->err = ctx->err;
    return code;
  };
  if (ctx == owner) return refuse("a context cannot attach to itself", VG_E_ARG);
  if (ctx->device != owner->device) return refuse("the contexts are on different devices", VG_E_ARG);
  if (memcmp(&ctx->cfg, &owner->cfg, sizeof(vg_config)) != 0)
    return refuse("the contexts' vg_config differ (they must be equal byte for byte)", VG_E_ARG);
  if (ctx->view_of) return refuse("the tracker is already attached (vg_map_detach first)", VG_E_STATE);
  if (ctx->views > 0) return refuse("the tracker is itself an owner (contexts are attached to it)", VG_E_STATE);
  if (owner->view_of) return refuse("the owner is itself attached to another context's map", VG_E_STATE);
  if (ctx->fleet || owner->fleet) return refuse("a fleet's tracker cannot attach or be attached to", VG_E_STATE);
  if (owner->mapping) return refuse("the owner is mapping (vg_set_mapping(owner, 0) first)", VG_E_STATE);
  if (sharded(ctx) || sharded(owner)) return refuse("a context is sharded", VG_E_STATE);
  if (hp(ctx)->in_scan || hp(owner)->in_scan) return refuse("a context is inside a scan (vg_step_end first)", VG_E_STATE);
  if (init_active(hp(owner))) return refuse("the owner's cold-start initialisation is still running", VG_E_STATE);
  VG_TRY(drain_all(owner));
  VG_TRY(drain_all(ctx));
  std::vector<unsigned char> blob;
  host_ckpt_blob(owner, blob);
  void* snap = nullptr;
  // the one thing the blob's parser checks against the receiving context's capacity, named here
  for (int i = 0; i < 32; i++)
    if (hp(owner)->wp_n[i] > ctx->cap.max_points_per_scan)
      return refuse("a scan of the owner's window is larger than the tracker's max_points_per_scan", VG_E_ARG);
  if (host_ckpt_parse(ctx, blob.data(), blob.size(), &snap) != VG_OK)
    return refuse("the owner's host state did not parse (host_ckpt_parse refused the blob host_ckpt_blob wrote)",
                  VG_E_STATE);
  // ---- every check passed: from here the tracker is rewritten
  int r = vg_reset(ctx);
  if (r != VG_OK) {
    host_ckpt_drop(snap);
    return r;
  }
  {
    DState* d = ctx->st;
    const DState* s = owner->st;
    hipError_t e = hipSuccess;
    auto field = [&](void* dst, const void* src, size_t bytes) {
      if (e == hipSuccess) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice);
    };
    field(d->xc, s->xc, sizeof(d->xc));
    field(d->xp, s->xp, sizeof(d->xp));
    field(d->G6, s->G6, sizeof(d->G6));
    field(d->nnt, s->nnt, sizeof(d->nnt));
    field(d->traj, s->traj, sizeof(d->traj));
    field(d->xs, s->xs, sizeof(d->xs));
    field(d->bias, s->bias, sizeof(d->bias));
    field(&d->jour, &s->jour, sizeof(double));
    field(d->last_pos, s->last_pos, sizeof(d->last_pos));
    field(d->imurec, s->imurec, sizeof(d->imurec));
    field(&d->imu_head, &s->imu_head, sizeof(int));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      host_ckpt_drop(snap);
      ctx->err = std::string(who) + ": " + hipGetErrorString(e);
      return VG_E_HIP;
    }
  }
  host_ckpt_install(ctx, snap);
  ctx->tail_a_valid = false;
  ctx->sync_tail_armed = false;
  ctx->mapping = false;
  graphs_drop(ctx);  // a graph captured on the tracker's own map (it stepped before) must not be replayed on the view
  ctx->own_map = ctx->map;
  ctx->map = owner->map;
  ctx->view_of = owner;
  owner->views++;
  return VG_OK;
}

// The tracker's own map comes back, empty as the attach's reset left it, and
// with it a fresh context (vg_reset): the window the tracker followed belongs
// to the owner's map and means nothing in an empty one. Mapping stays off.
int host_map_detach(vg_ctx* ctx) {
  if (!ctx->view_of) {
    ctx->err = "vg_map_detach: the context is not attached";
    return VG_E_STATE;
  }
  VG_TRY(refuse_fleet(ctx, "vg_map_detach"));
  if (hp(ctx)->in_scan) {
    ctx->err = "vg_map_detach inside a scan (vg_step_end first)";
    return VG_E_STATE;
  }
  (void)drain_all(ctx);  // (a deferred error goes with the state the reset drops)
  (void)hipStreamSynchronize(ctx->stream);  // nothing of the tracker's reads the owner's map past this point
  graphs_drop(ctx);  // the IEKF graph captured while attached holds the owner's pointers
  ctx->map = ctx->own_map;
  ctx->view_of->views--;
  ctx->view_of = nullptr;
  return vg_reset(ctx);
}

int host_score_poses(vg_ctx* ctx, const float* xyz, int n, const double* poses, int K, const double* pose_var,
                     vg_pose_score* out, void* per_point) {
  if (ctx->shard.world > 1) {
    ctx->err = "vg_score_poses: the context is sharded (world > 1)";
    return VG_E_STATE;
  }
  VG_TRY(host_quiesce(ctx));
  return score_poses_dev(ctx, hp(ctx)->mpd, xyz, n, poses, K, pose_var, out, per_point);
}

// ---- the hypothesis grid (vina_gpu.h vg_reloc_grid)
static bool axis_count(double half, double step, int* n) {
  if (!(half >= 0.0) || !(step >= 0.0) || !std::isfinite(half) || !std::isfinite(step)) return false;
  if (half == 0.0 || step == 0.0) {
    *n = 0;
    return true;
  }
  const double k = std::floor(half / step + 1e-9);
  if (k > 1e6) return false;
  *n = (int)k;
  return true;
}
int reloc_grid(const vg_reloc_params* prm, double* out, int cap, int* count) {
  int hx, hz, hyaw;
  if (!axis_count(prm->half_xy, prm->step_xy, &hx) || !axis_count(prm->half_z, prm->step_z, &hz) ||
      !axis_count(prm->half_yaw, prm->step_yaw, &hyaw))
    return VG_E_ARG;
  const long long nx = 2 * hx + 1, nz = 2 * hz + 1, nyaw = 2 * hyaw + 1;
  const long long total = nx * nx * nz * nyaw;
  if (total > VG_SCORE_MAX_POSES) return VG_E_ARG;
  *count = (int)total;
  if (!out) return VG_OK;
  int k = 0;
  const int nb = (int)((nx + 3) / 4);
  for (int iz = -hz; iz <= hz; iz++)
    for (int iw = -hyaw; iw <= hyaw; iw++)
      for (int by = 0; by < nb; by++)
        for (int bx = 0; bx < nb; bx++)
          for (int j = 4 * by; j < 4 * by + 4 && j < nx; j++)
            for (int i = 4 * bx; i < 4 * bx + 4 && i < nx; i++, k++) {
              if (k >= cap) continue;
              out[4 * k] = (i - hx) * prm->step_xy;
              out[4 * k + 1] = (j - hx) * prm->step_xy;
              out[4 * k + 2] = iz * prm->step_z;
              out[4 * k + 3] = iw * prm->step_yaw;
            }
  return VG_OK;
}

// more matches first, then the lower cost per match
static bool better(const vg_pose_score& a, const vg_pose_score& b) {
  if (a.matches != b.matches) return a.matches > b.matches;
  const double ca = a.matches > 0 ? a.cost / a.matches : 0.0, cb = b.matches > 0 ? b.cost / b.matches : 0.0;
  return ca < cb;
}

// H x = b, H symmetric 6 x 6 (packed upper, the IEKF's HTH order): Gaussian
// elimination with partial pivoting; false when singular to working precision
bool solve6(const double* hth, const double* b, double* x) {
  double A[6][7];
  int k = 0;
  double scale = 0.0;
  for (int r = 0; r < 6; r++)
    for (int c = r; c < 6; c++, k++) {
      A[r][c] = A[c][r] = hth[k];
      scale = std::max(scale, std::fabs(hth[k]));
    }
  for (int r = 0; r < 6; r++) A[r][6] = b[r];
  if (!(scale > 0.0) || !std::isfinite(scale)) return false;
  for (int c = 0; c < 6; c++) {
    int p = c;
    for (int r = c + 1; r < 6; r++)
      if (std::fabs(A[r][c]) > std::fabs(A[p][c])) p = r;
    if (!(std::fabs(A[p][c]) > 1e-13 * scale)) return false;
    if (p != c)
      for (int j = 0; j < 7; j++) std::swap(A[p][j], A[c][j]);
    for (int r = c + 1; r < 6; r++) {
      const double f = A[r][c] / A[c][c];
      for (int j = c; j < 7; j++) A[r][j] -= f * A[c][j];
    }
  }
  for (int r = 5; r >= 0; r--) {
    double s = A[r][6];
    for (int j = r + 1; j < 6; j++) s -= A[r][j] * x[j];
    x[r] = s / A[r][r];
  }
  for (int r = 0; r < 6; r++)
    if (!std::isfinite(x[r])) return false;
  return true;
}

bool reloc_better(const vg_pose_score& a, const vg_pose_score& b) { return better(a, b); }

// x_curr takes the pose with the initial covariance; v, bg, ba and g stay
int reloc_install(vg_ctx* ctx, const double* pose12) {
  HX& x = hp(ctx)->x_curr;
  memcpy(x.R.a, pose12, 72);
  memcpy(x.p.a, pose12 + 9, 24);
  x.cov = HX().cov;  // the initial covariance (imu_ekf.cpp)
  double blk[kXC];
  hx_put_block(x, blk);  // the device's copy too (a scan that propagates on the device starts from it)
  VG_HIP(hipMemcpy(ctx->st->xc, blk, sizeof(blk), hipMemcpyHostToDevice));
  return VG_OK;
}

int host_relocalize(vg_ctx* ctx, const float* xyz, int n, const double* guess, const vg_reloc_params* prm,
                    int install, double* out_pose, vg_pose_score* out_score, int* ok) {
  HostPipe* P = hp(ctx);
  if (P->in_scan) {
    ctx->err = "vg_relocalize inside a scan (vg_step_end first)";
    return VG_E_STATE;
  }
  if (ctx->shard.world > 1) {
    ctx->err = "vg_relocalize: the context is sharded (world > 1)";
    return VG_E_STATE;
  }
  int K = 0;
  if (reloc_grid(prm, nullptr, 0, &K) != VG_OK) {
    ctx->err = "vg_relocalize: bad search window (negative, or more than 65,536 hypotheses)";
    return VG_E_ARG;
  }
  VG_TRY(host_sync(ctx));
  const MP& mp = P->mpd;
  const int top = prm->refine_top > 0 ? prm->refine_top : 8;
  const int iters = prm->refine_iters > 0 ? prm->refine_iters : 8;
  const double ratio = prm->min_match_ratio > 0 ? prm->min_match_ratio : 0.5;
  std::vector<double> off((size_t)K * 4), poses((size_t)K * 12);
  reloc_grid(prm, off.data(), K, &K);
  // yaw: about the gravity direction of the context's state (up = -g / |g|)
  V3 up = scl(P->x_curr.g, -1.0);
  const double gn = norm3(up);
  up = gn > 0 ? scl(up, 1.0 / gn) : v3(0, 0, 1);
  M3 Rg;
  memcpy(Rg.a, guess, 72);
  for (int k = 0; k < K; k++) {
    const M3 R = mul(Exp(scl(up, off[4 * k + 3])), Rg);
    memcpy(&poses[(size_t)k * 12], R.a, 72);
    for (int j = 0; j < 3; j++) poses[(size_t)k * 12 + 9 + j] = guess[9 + j] + off[4 * k + j];
  }
  std::vector<vg_pose_score> sc((size_t)K);
  VG_TRY(score_poses_dev(ctx, mp, xyz, n, poses.data(), K, nullptr, sc.data(), nullptr));
  std::vector<int> order((size_t)K);
  for (int k = 0; k < K; k++) order[k] = k;
  const int keep = std::min(top, K);
  std::partial_sort(order.begin(), order.begin() + keep, order.end(), [&](int a, int b) {
    if (better(sc[a], sc[b])) return true;
    if (better(sc[b], sc[a])) return false;
    return a < b;
  });
  // LiDAR-only Gauss-Newton on (rotation, position): dx = HTH^-1 HTz of the
  // IEKF's sums, R <- R Exp(dx[0:3]), p += dx[3:6] (the IEKF update's boxplus)
  double best_pose[12];
  vg_pose_score best;
  memset(&best, 0, sizeof(best));
  bool have = false;
  for (int t = 0; t < keep; t++) {
    double pose[12];
    memcpy(pose, &poses[(size_t)order[t] * 12], sizeof(pose));
    for (int it = 0; it < iters; it++) {
      double s34[34], dx[6];
      VG_TRY(score_normal_dev(ctx, mp, pose, nullptr, s34));
      if (s34[33] < 6 || !solve6(s34, s34 + 21, dx)) break;
      M3 R;
      memcpy(R.a, pose, 72);
      R = mul(R, Exp(v3(dx[0], dx[1], dx[2])));
      memcpy(pose, R.a, 72);
      for (int j = 0; j < 3; j++) pose[9 + j] += dx[3 + j];
      if (norm3(v3(dx[0], dx[1], dx[2])) < 1e-7 && norm3(v3(dx[3], dx[4], dx[5])) < 1e-6) break;
    }
    vg_pose_score r;
    VG_TRY(score_poses_dev(ctx, mp, nullptr, n, pose, 1, nullptr, &r, nullptr));
    if (!have || better(r, best)) {
      best = r;
      memcpy(best_pose, pose, sizeof(pose));
      have = true;
    }
  }
  if (!have) memcpy(best_pose, guess, sizeof(best_pose));
  const bool good = have && n > 0 && (double)best.matches >= ratio * n;
  memcpy(out_pose, best_pose, sizeof(best_pose));
  if (out_score) *out_score = best;
  *ok = good ? 1 : 0;
  if (good && install) VG_TRY(reloc_install(ctx, best_pose));
  return VG_OK;
}

}  // namespace vg

extern "C" {
int vg_set_mapping(vg_ctx* ctx, int on) {
  if (!ctx) return VG_E_ARG;
  return vg::host_set_mapping(ctx, on);
}
int vg_map_attach(vg_ctx* tracker, vg_ctx* owner) {
  if (!tracker || !owner) return VG_E_ARG;
  return vg::host_map_attach(tracker, owner);
}
int vg_map_detach(vg_ctx* tracker) {
  if (!tracker) return VG_E_ARG;
  return vg::host_map_detach(tracker);
}
int vg_score_poses(vg_ctx* ctx, const float* xyz, int n, const double* poses, int K, const double* pose_var,
                   vg_pose_score* out, void* per_point) {
  if (!ctx || n < 0 || K <= 0 || K > VG_SCORE_MAX_POSES || !poses || !out || (n > 0 && !xyz) ||
      (per_point && K != 1) || n > ctx->cap.max_points_per_scan)
    return VG_E_ARG;
  static const float none[3] = {0, 0, 0};
  return vg::host_score_poses(ctx, n > 0 ? xyz : none, n, poses, K, pose_var, out, per_point);
}
int vg_reloc_grid(const vg_reloc_params* prm, double* out, int cap, int* count) {
  if (!prm || !count || cap < 0) return VG_E_ARG;
  return vg::reloc_grid(prm, out, cap, count);
}
int vg_relocalize(vg_ctx* ctx, const float* xyz, int n, const double* guess_pose, const vg_reloc_params* prm,
                  int install, double* out_pose, vg_pose_score* out_score, int* ok) {
  if (!ctx || n < 0 || (n > 0 && !xyz) || !guess_pose || !prm || !out_pose || !ok ||
      n > ctx->cap.max_points_per_scan)
    return VG_E_ARG;
  static const float none[3] = {0, 0, 0};
  return vg::host_relocalize(ctx, n > 0 ? xyz : none, n, guess_pose, prm, install, out_pose, out_score, ok);
}
}
