// localizability_host.cpp — vg_localizability and vg_scan_info, host side: the
// argument checks, the drain of outstanding work, and the pose vg_scan_info
// defaults to (the kernels and their staging: localizability.hip).
#include <cstring>

#include "vg_host.h"
#include "vg_query.h"

namespace vg {

int host_localizability(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D,
                        const vg_info_params* prm, vg_info_rec* out) {
  VG_TRY(query_open(ctx, "vg_localizability"));
  return localizability_dev(ctx, hp(ctx)->mpd, positions, M, dirs, D, prm, out);
}

int host_scan_info(vg_ctx* ctx, const float* xyz, int n, const double* pose12, const vg_diff_params* diff,
                   const vg_info_params* prm, vg_info_rec* out) {
  VG_TRY(query_open(ctx, "vg_scan_info"));
  double pose[12];
  if (pose12) {
    memcpy(pose, pose12, sizeof(pose));
  } else {  // the context's current state (the host mirror, current after the drain)
    const HX& x = hp(ctx)->x_curr;
    memcpy(pose, x.R.a, 72);
    memcpy(pose + 9, x.p.a, 24);
  }
  return scan_info_dev(ctx, hp(ctx)->mpd, xyz, n, pose, diff, prm, out);
}

}  // namespace vg

extern "C" {
int vg_localizability(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D,
                      const vg_info_params* prm, vg_info_rec* out) {
  if (!ctx || M < 0 || D < 1 || D > vg::kInfoMaxDirs || !dirs) return VG_E_ARG;
  if (M == 0) return VG_OK;
  if (!positions || !out) return VG_E_ARG;
  return vg::host_localizability(ctx, positions, M, dirs, D, prm, out);
}
int vg_scan_info(vg_ctx* ctx, const float* xyz, int n, const double* pose12, const vg_diff_params* diff,
                 const vg_info_params* prm, vg_info_rec* out) {
  if (!ctx || n < 0 || !out || (n > 0 && !xyz) || n > ctx->cap.max_points_per_scan) return VG_E_ARG;
  return vg::host_scan_info(ctx, xyz, n, pose12, diff, prm, out);
}
}
