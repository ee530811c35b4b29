// vg_occ.h — one traced ray rasterised into the occupancy grid's two count
// planes (vina_gpu.h "Occupancy grid"; occupancy.hip's k_occ_cast). The ray's
// record comes from ray_trace (vg_ray.h), unchanged; this file only walks the
// 2-D lattice.
//
// The free segment. (ta, tb) = (max(t_min, 0), r_end), cut to the t on which
// z_lo <= t d_z <= z_hi (one division per band limit; d_z = 0: all t or none),
// then cut to the grid grown by one cell per side (the slab test per axis).
// The last cut changes no mark, marks outside the grid being dropped, and its
// rounding falls a cell away from the grid; it bounds the walk by nx + ny + 8
// cells wherever the origin lies.
//
// The walk. Amanatides-Woo in double on the lattice x0 + k res, y0 + k res,
// from the cell of the segment's first point: a cell's exit is ((k + 1 | k) res
// + x0 - o_x) / d_x of the axis, taken from the lattice line itself and never
// accumulated, as ray_walk does (equal exits: x first). A cell is marked when
// its piece of the segment has t_out > t_in, so a ray through a lattice corner
// marks neither diagonal neighbour, and a first point that rounding put on the
// wrong side of a line costs a piece of zero length, not a mark. The cells of a
// straight walk are distinct: a ray marks a cell at most once without any
// bookkeeping. An axis with d = 0 never steps (its exit is +inf); with both
// zero the ray marks the cell it stands in. No stack, no private array.
#pragma once
#include "vg_diff.h"

namespace vg {

constexpr int kOccBlock = kRayBlock;  // 256 threads
constexpr int kOccEnded = kRayTruncated | kRayLeftRange | kRayInvalid;  // such a ray marks nothing

struct OccPrm {  // vg_occ_params with the defaults applied
  RayPrm ray;
  double x0, y0, res;
  double z_lo, z_hi, free_on_miss;
  double occ_ratio;  // <= 0: off
  int nx, ny;
  int min_occ, min_free;
  int flags, pad;
};
inline OccPrm occ_prm(const vg_occ_params* p) {
  OccPrm q;
  q.ray = ray_prm(&p->ray);
  q.x0 = p->x0, q.y0 = p->y0, q.res = p->res;
  q.z_lo = p->z_lo, q.z_hi = p->z_hi;
  q.free_on_miss = p->free_on_miss > 0.0 ? p->free_on_miss : 0.0;
  q.occ_ratio = p->occ_ratio > 0.0 ? p->occ_ratio : 0.0;
  q.nx = p->nx, q.ny = p->ny;
  q.min_occ = p->min_occ > 0 ? p->min_occ : 1;
  q.min_free = p->min_free > 0 ? p->min_free : 1;
  q.flags = p->flags;
  q.pad = 0;
  return q;
}

// floor((v - g0) / res) as an int, held to [-4, n + 4] (a cell outside the grid is only ever compared)
__device__ __forceinline__ int occ_cell(double v, double g0, double res, int n) {
  const double c = floor((v - g0) / res);
  return c >= -4.0 ? (c <= (double)(n + 4) ? (int)c : n + 4) : -4;  // (a NaN lands on -4: outside)
}

// the slab cut of (ta, tb) to [lo, hi] along one axis; false: nothing is left
__device__ __forceinline__ bool occ_clip(double o, double d, double lo, double hi, double& ta, double& tb) {
  if (d == 0.0) return o >= lo && o <= hi;
  const double t1 = (lo - o) / d, t2 = (hi - o) / d;
  const double tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
  ta = tn > ta ? tn : ta;
  tb = tf < tb ? tf : tb;
  return ta < tb;
}

// o, dir: the ray as ray_trace took it; h: its record. Adds the ray's marks to n_free / n_occ (nx ny ints
// each); in_band: the ray marks and its hit lies in the band
__device__ __forceinline__ void occ_ray(const OccPrm& q, const V3& o, const V3& dir, const vg_ray_hit& h,
                                        int* __restrict__ n_free, int* __restrict__ n_occ, bool& in_band) {
  in_band = false;
  if (h.flags & kOccEnded) return;
  const bool hit = (h.flags & kRayHit) != 0;
  if (!hit && !(q.free_on_miss > 0.0)) return;
  const double r_end = hit ? h.range : q.free_on_miss;
  const double dn = norm3(dir);  // (ray_trace's own normalisation)
  const double dx = dir[0] / dn, dy = dir[1] / dn, dz = dir[2] / dn;
  int hcx = -8, hcy = -8;  // the in-band hit's cell (-8: none, or outside the grid)
  if (hit) {
    const double rz = h.range * dz;
    if (rz >= q.z_lo && rz <= q.z_hi) {
      in_band = true;
      const int cx = occ_cell(o[0] + h.range * dx, q.x0, q.res, q.nx);
      const int cy = occ_cell(o[1] + h.range * dy, q.y0, q.res, q.ny);
      if (cx >= 0 && cx < q.nx && cy >= 0 && cy < q.ny) {
        hcx = cx, hcy = cy;
        atomicAdd(&n_occ[(size_t)cy * q.nx + cx], 1);
      }
    }
  }
  if ((q.flags & 1) && (h.flags & kRayOccupied)) return;
  // the free segment: the ray's interval, the band, the grid grown by a cell
  double ta = q.ray.t_min > 0.0 ? q.ray.t_min : 0.0, tb = r_end;
  if (dz != 0.0) {
    const double a = q.z_lo / dz, b = q.z_hi / dz;
    const double lo = dz > 0.0 ? a : b, hi = dz > 0.0 ? b : a;
    ta = lo > ta ? lo : ta;
    tb = hi < tb ? hi : tb;
  } else if (!(q.z_lo <= 0.0 && 0.0 <= q.z_hi)) {
    return;
  }
  if (!(ta < tb)) return;
  if (!occ_clip(o[0], dx, q.x0 - q.res, q.x0 + (double)(q.nx + 1) * q.res, ta, tb)) return;
  if (!occ_clip(o[1], dy, q.y0 - q.res, q.y0 + (double)(q.ny + 1) * q.res, ta, tb)) return;
  if (!(ta < tb)) return;
  const int sx = dx > 0.0 ? 1 : (dx < 0.0 ? -1 : 0), sy = dy > 0.0 ? 1 : (dy < 0.0 ? -1 : 0);
  int kx = occ_cell(o[0] + ta * dx, q.x0, q.res, q.nx), ky = occ_cell(o[1] + ta * dy, q.y0, q.res, q.ny);
  double tnx = sx ? (((double)(kx + (sx > 0 ? 1 : 0)) * q.res + q.x0) - o[0]) / dx : __builtin_huge_val();
  double tny = sy ? (((double)(ky + (sy > 0 ? 1 : 0)) * q.res + q.y0) - o[1]) / dy : __builtin_huge_val();
  double t_in = ta;
  for (int step = q.nx + q.ny + 16; step > 0; step--) {  // (the cut bounds the walk; the count only backs it)
    const bool along_y = tny < tnx;
    const double t_exit = along_y ? tny : tnx;
    const double t_out = t_exit < tb ? t_exit : tb;
    if (t_out > t_in && kx >= 0 && kx < q.nx && ky >= 0 && ky < q.ny && !(kx == hcx && ky == hcy))
      atomicAdd(&n_free[(size_t)ky * q.nx + kx], 1);
    if (!(t_exit < tb)) break;  // (both axes still: t_exit = +inf, the one cell was marked)
    t_in = t_exit > t_in ? t_exit : t_in;
    if (along_y) {
      ky += sy;
      tny = (((double)(ky + (sy > 0 ? 1 : 0)) * q.res + q.y0) - o[1]) / dy;
    } else {
      kx += sx;
      tnx = (((double)(kx + (sx > 0 ? 1 : 0)) * q.res + q.x0) - o[0]) / dx;
    }
  }
}

}  // namespace vg
