// raycast_host.cpp — vg_raycast and vg_scan_diff, host side: the argument
// checks, the drain of outstanding work, and the pose vg_scan_diff defaults to
// (the kernels and their staging: raycast.hip).
#include <cstring>

#include "vg_host.h"

namespace vg {

static int ray_allowed(vg_ctx* ctx, const char* who) {
  if (ctx->shard.world > 1) {
    ctx->err = std::string(who) + ": the context is sharded (world > 1)";
    return VG_E_STATE;
  }
  return host_quiesce(ctx);
}

int host_raycast(vg_ctx* ctx, const double* origins, int n_origins, const double* dirs, int n,
                 const vg_ray_params* prm, vg_ray_hit* out) {
  VG_TRY(ray_allowed(ctx, "vg_raycast"));
  return raycast_dev(ctx, hp(ctx)->mpd, origins, n_origins, dirs, n, prm, out);
}

int host_scan_diff(vg_ctx* ctx, const float* xyz, int n, const double* pose12, const vg_diff_params* prm,
                   vg_diff_point* per_point, vg_diff_summary* out) {
  VG_TRY(ray_allowed(ctx, "vg_scan_diff"));
  double pose[12];
  if (pose12) {
    memcpy(pose, pose12, sizeof(pose));
  } else {  // the context's current state (the host mirror, current after the drain)
    const HX& x = hp(ctx)->x_curr;
    memcpy(pose, x.R.a, 72);
    memcpy(pose + 9, x.p.a, 24);
  }
  return scan_diff_dev(ctx, hp(ctx)->mpd, xyz, n, pose, prm, per_point, out);
}

}  // namespace vg

extern "C" {
int vg_raycast(vg_ctx* ctx, const double* origins, int n_origins, const double* dirs, int n,
               const vg_ray_params* prm, vg_ray_hit* out) {
  if (!ctx || n < 0) return VG_E_ARG;
  if (n == 0) return n_origins == 0 || n_origins == 1 ? VG_OK : VG_E_ARG;
  if (!origins || !dirs || !out || (n_origins != 1 && n_origins != n)) return VG_E_ARG;
  return vg::host_raycast(ctx, origins, n_origins, dirs, n, prm, out);
}
int vg_scan_diff(vg_ctx* ctx, const float* xyz, int n, const double* pose12, const vg_diff_params* prm,
                 vg_diff_point* per_point, vg_diff_summary* out) {
  if (!ctx || n < 0 || !out || (n > 0 && !xyz) || n > ctx->cap.max_points_per_scan) return VG_E_ARG;
  return vg::host_scan_diff(ctx, xyz, n, pose12, prm, per_point, out);
}
}
