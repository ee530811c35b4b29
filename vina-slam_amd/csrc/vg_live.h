// vg_live.h — one scan point's record for the live obstacle layer (vina_gpu.h
// "Live obstacle layer"; live.hip's k_live_points): the class from vg_diff.h's
// diff_point, the body k_scan_diff runs, then the point's flags and its three
// cells in double. Reads the map only; writes nothing but the record.
#pragma once
#include "vg_diff.h"

namespace vg {

constexpr int kLiveCellMax = 1 << 30;  // a cell index is held to [-2^30, 2^30]: n stays <= 4097, nothing overflows

// floor((v - g0) / res) as an int, held to +-kLiveCellMax (v finite)
__device__ __forceinline__ int live_cell(double v, double g0, double res) {
  const double c = floor((v - g0) / res);
  return c >= -(double)kLiveCellMax ? (c <= (double)kLiveCellMax ? (int)c : kLiveCellMax) : -kLiveCellMax;
}

__device__ __forceinline__ bool live_finite(const V3& v) {
  return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]);
}

// pb: the point in the LiDAR frame; rec: its record; rflags: the ray's flags (diff_wave_counts takes them)
__device__ __forceinline__ void live_point(const MP& mp, const DevMap& m, const V3& pb, const Pose12& pose,
                                           const DiffPrm& prm, const LivePrm& q, vg_live_point& rec, int& rflags) {
  vg_diff_point dp;
  double av;
  V3 w, o;
  vg_ray_hit h;
  diff_point(mp, m, pb, pose, prm, dp, av, rflags, w, o, h);
  rec.cls = dp.cls;
  rec.flags = 0;
  rec.ax = rec.ay = rec.bx = rec.by = rec.mx = rec.my = 0;
  if (!live_finite(o) || !live_finite(w)) return;
  const double r = dp.r_meas;
  const double dz = w[2] - o[2];
  int flags = 0;
  const bool in_band = q.z_lo <= dz && dz <= q.z_hi;
  if (in_band) flags |= VG_LIVE_IN_BAND;
  const bool cls_marks = dp.cls == VG_DIFF_APPEARED || (q.unknown_marks && dp.cls == VG_DIFF_UNKNOWN);
  if (cls_marks && in_band && q.r_min <= r && r <= q.mark_max) flags |= VG_LIVE_MARKS;
  rec.mx = live_cell(w[0], q.x0, q.res);
  rec.my = live_cell(w[1], q.y0, q.res);
  if (r > 0.0) {
    double t_b = r;
    if (q.clear_max < t_b) t_b = q.clear_max, flags |= VG_LIVE_CUT;
    if (dz != 0.0) {
      const double t_z = (dz > 0.0 ? q.z_hi : q.z_lo) * r / dz;
      if (t_z < t_b) t_b = t_z, flags = (flags & ~VG_LIVE_CUT) | VG_LIVE_LEFT_BAND;
    }
    const double f = t_b / r;
    const double ex = o[0] + f * (w[0] - o[0]), ey = o[1] + f * (w[1] - o[1]);
    flags |= VG_LIVE_CLEARS;
    rec.ax = live_cell(o[0], q.x0, q.res);
    rec.ay = live_cell(o[1], q.y0, q.res);
    rec.bx = live_cell(ex, q.x0, q.res);
    rec.by = live_cell(ey, q.y0, q.res);
  }
  rec.flags = flags;
}

}  // namespace vg
