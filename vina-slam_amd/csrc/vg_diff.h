// vg_diff.h — one scan point against the range the map expects along its beam
// (vina_gpu.h vg_scan_diff): the per-point body shared by k_scan_diff
// (raycast.hip) and k_change_accum (change.hip), which therefore give the same
// bits. Reads the map only, through the traversal of vg_ray.h.
#pragma once
#include "vg_ray.h"

namespace vg {

constexpr int kRayBlock = 256;

struct Pose12 {
  double v[12];
};

struct DiffPrm {  // vg_diff_params with the defaults applied
  RayPrm ray;
  double gate_sigma, gate_floor;
};

inline RayPrm ray_prm(const vg_ray_params* p) {
  RayPrm q;
  q.t_min = p ? p->t_min : 0.0;
  q.t_max = p && p->t_max > 0.0 ? p->t_max : 100.0;
  q.min_cos = p && p->min_cos > 0.0 ? p->min_cos : 0.05;
  q.max_steps = p && p->max_steps > 0 ? p->max_steps : 4096;
  q.pad = 0;
  return q;
}
inline DiffPrm diff_prm(const vg_diff_params* p) {
  DiffPrm q;
  q.ray = ray_prm(p ? &p->ray : nullptr);
  q.gate_sigma = p && p->gate_sigma > 0.0 ? p->gate_sigma : 3.0;
  q.gate_floor = p && p->gate_floor > 0.0 ? p->gate_floor : 0.0;
  return q;
}

// pb: the point in the LiDAR frame. dp: its record; av: |range - r| where
// consistent, else 0; rflags: the ray's flags; w: the point in the world;
// o, h: the sensor origin and the beam's hit record (vg_info.h sums over them)
__device__ __forceinline__ void diff_point(const MP& mp, const DevMap& m, const V3& pb, const Pose12& pose,
                                           const DiffPrm& prm, vg_diff_point& dp, double& av, int& rflags, V3& w,
                                           V3& o, vg_ray_hit& h) {
  const M3 R = ld_m3(pose.v);
  const V3 p = ld_v3(pose.v + 9);
  o = rigid(R, ld_v3(mp.extt), p);
  w = rigid(R, rigid(ld_m3(mp.extR), pb, ld_v3(mp.extt)), p);
  const V3 dv = sub(w, o);
  const double r = norm3(dv);
  const double dept2 = (double)mp.dept * (double)mp.dept, beam2 = r * r * mp.beam_dv;
  const double mc2 = prm.ray.min_cos * prm.ray.min_cos;
  RayPrm q = prm.ray;
  const double reach = r + (prm.gate_sigma * sqrt(dept2 + beam2 * (1.0 - mc2) / mc2) + 1.0);
  if (reach < q.t_max) q.t_max = reach;
  ray_trace(m, mp.vs, o, dv, q, h);
  rflags = h.flags;
  dp.cls = VG_DIFF_UNKNOWN;
  dp.leaf = -1;
  dp.r_meas = r;
  dp.r_map = 0.0;
  dp.gate = 0.0;
  av = 0.0;
  if (h.flags & kRayHit) {
    const double c2 = h.ndotd * h.ndotd;
    double g2 = prm.gate_sigma * prm.gate_sigma * (h.var + dept2 + beam2 * (1.0 - c2) / c2);
    const double f2 = prm.gate_floor * prm.gate_floor;
    if (!(g2 >= f2)) g2 = f2;
    const double gate = sqrt(g2), diff = h.range - r;
    dp.leaf = h.leaf;
    dp.r_map = h.range;
    dp.gate = gate;
    if (fabs(diff) <= gate) {
      dp.cls = VG_DIFF_CONSISTENT;
      av = fabs(diff);
    } else {
      dp.cls = diff > gate ? VG_DIFF_APPEARED : VG_DIFF_VANISHED;
    }
  }
}
__device__ __forceinline__ void diff_point(const MP& mp, const DevMap& m, const V3& pb, const Pose12& pose,
                                           const DiffPrm& prm, vg_diff_point& dp, double& av, int& rflags, V3& w) {
  V3 o;
  vg_ray_hit h;
  diff_point(mp, m, pb, pose, prm, dp, av, rflags, w, o, h);
}

// the wave's counts into the summary's six ints: one atomic per class that
// occurs. Every lane of the wave calls it (cls -1: no point)
__device__ __forceinline__ void diff_wave_counts(int cls, bool valid, int rflags, int* __restrict__ sum) {
  const int lane = threadIdx.x & 63;
  for (int c = 0; c < 6; c++) {
    const bool mine = c < 4 ? cls == c : (valid && (rflags & (c == 4 ? kRayTruncated : kRayOccupied)) != 0);
    const unsigned long long b = __ballot(mine);
    if (lane == 0 && b) atomicAdd(&sum[c], __popcll(b));
  }
}

}  // namespace vg
