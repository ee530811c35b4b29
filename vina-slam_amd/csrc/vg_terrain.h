// vg_terrain.h — one traced ray of the terrain layer (vina_gpu.h "Terrain
// layer"; terrain.hip's k_ter_ground and k_ter_marks): the ground mark of pass
// 1 and the walk with a ground reference of pass 2. The record comes from
// ray_trace (vg_ray.h), the cell and the slab cut from vg_occ.h, both unchanged.
//
// Heights are quantised once per use: ter_q is floor(z / z_res) held to +-2^30,
// so that every difference of two of them fits an int and |q| = 2^30 reads "out
// of range" (ter_in_range).
//
// The walk is occ_ray's (Amanatides-Woo in double, exits taken from the lattice
// line itself, a piece marks when t_out > t_in) without the origin band: the
// segment is (max(t_min, 0), r_end) cut to the grid grown by a cell. Per piece
// inside the grid one load of elev (L2-served: the lanes of a wave fan out from
// one origin) moves the reference, one quantisation judges the piece. The free
// mark of the hit's own cell is held in a flag until the hit has been judged
// against the reference the walk ended with; the cells of a straight walk are
// distinct, so one flag is enough.
#pragma once
#include "vg_occ.h"

namespace vg {

constexpr int kTerLimit = 1 << 30;  // |q| >= this: out of range
constexpr int kTerNone = INT32_MIN;

struct TerPrm {  // vg_terrain_params with the defaults applied
  RayPrm ray;
  double x0, y0, res;
  double free_on_miss, occ_ratio;
  double z_res, up_min, g_lo, g_hi, sensor_height;
  int nx, ny;
  int min_occ, min_free, min_ground, flags;
  int clo, chi, smax, pad;  // q(clear_lo), q(clear_hi), q(step_max)
};

// floor(z / z_res) held to [-2^30, 2^30] (a NaN lands on -2^30: out of range)
__host__ __device__ __forceinline__ int ter_q(double z, double z_res) {
  const double c = floor(z / z_res);
  return c > -(double)kTerLimit ? (c < (double)kTerLimit ? (int)c : kTerLimit) : -kTerLimit;
}
__host__ __device__ __forceinline__ bool ter_in_range(int q) { return q > -kTerLimit && q < kTerLimit; }

inline TerPrm ter_prm(const vg_terrain_params* p) {
  TerPrm q;
  q.ray = ray_prm(&p->ray);
  q.x0 = p->x0, q.y0 = p->y0, q.res = p->res;
  q.free_on_miss = p->free_on_miss > 0.0 ? p->free_on_miss : 0.0;
  q.occ_ratio = p->occ_ratio > 0.0 ? p->occ_ratio : 0.0;
  q.z_res = p->z_res > 0.0 ? p->z_res : 0.001;
  q.up_min = p->up_min > 0.0 ? p->up_min : 0.8191520442889918;  // cos 35 deg
  const bool g0 = p->g_lo == 0.0 && p->g_hi == 0.0, c0 = p->clear_lo == 0.0 && p->clear_hi == 0.0;
  q.g_lo = g0 ? -3.0 : p->g_lo, q.g_hi = g0 ? -0.1 : p->g_hi;
  q.sensor_height = p->sensor_height;
  q.nx = p->nx, q.ny = p->ny;
  q.min_occ = p->min_occ > 0 ? p->min_occ : 1;
  q.min_free = p->min_free > 0 ? p->min_free : 1;
  q.min_ground = p->min_ground > 0 ? p->min_ground : 1;
  q.flags = p->flags;
  q.clo = ter_q(c0 ? 0.15 : p->clear_lo, q.z_res);
  q.chi = ter_q(c0 ? 1.5 : p->clear_hi, q.z_res);
  q.smax = (p->flags & 2) ? ter_q(p->step_max, q.z_res) : 0;
  q.pad = 0;
  return q;
}

// clo <= a - ref <= chi, both heights in range (the difference of two held values fits an int)
__device__ __forceinline__ bool ter_band(const TerPrm& q, int a, int ref) {
  if (!ter_in_range(a)) return false;
  const int d = a - ref;
  return d >= q.clo && d <= q.chi;
}

// Pass 1. o, dir: the ray as ray_trace took it; h: its record. Adds the ray's ground hit to the four planes
// (nx ny each); ground: it had one; out_of_range: it marks, hit, and q(h_z) is out of range
__device__ __forceinline__ void ter_ground(const TerPrm& q, const V3& o, const V3& dir, const vg_ray_hit& h,
                                           int* __restrict__ g_n, unsigned long long* __restrict__ g_sum,
                                           int* __restrict__ g_min, int* __restrict__ g_max, bool& ground,
                                           bool& out_of_range) {
  ground = out_of_range = false;
  if ((h.flags & kOccEnded) || !(h.flags & kRayHit)) return;
  const double dn = norm3(dir);  // (ray_trace's own normalisation)
  const double dx = dir[0] / dn, dy = dir[1] / dn, dz = dir[2] / dn;
  const int qz = ter_q(o[2] + h.range * dz, q.z_res);
  if (!ter_in_range(qz)) {
    out_of_range = true;
    return;
  }
  const double rz = h.range * dz;
  if (!(dz < 0.0) || !(fabs(h.normal[2]) >= q.up_min) || !(rz >= q.g_lo && rz <= q.g_hi)) return;
  const int cx = occ_cell(o[0] + h.range * dx, q.x0, q.res, q.nx);
  const int cy = occ_cell(o[1] + h.range * dy, q.y0, q.res, q.ny);
  if (!(cx >= 0 && cx < q.nx && cy >= 0 && cy < q.ny)) return;
  const size_t i = (size_t)cy * q.nx + cx;
  ground = true;
  atomicAdd(&g_n[i], 1);
  atomicAdd(&g_sum[i], (unsigned long long)(long long)qz);  // (two's complement: the sum of signed terms)
  atomicMin(&g_min[i], qz);
  atomicMax(&g_max[i], qz);
}

// Pass 2. Adds the ray's marks to n_free / n_occ (nx ny ints each), reading elev (nx ny); in_band: the ray
// marks and its hit lies in the band above its reference
__device__ __forceinline__ void ter_marks(const TerPrm& q, const V3& o, const V3& dir, const vg_ray_hit& h,
                                          const int* __restrict__ elev, int* __restrict__ n_free,
                                          int* __restrict__ n_occ, bool& in_band) {
  in_band = false;
  if (h.flags & kOccEnded) return;
  const bool hit = (h.flags & kRayHit) != 0;
  if (!hit && !(q.free_on_miss > 0.0)) return;
  const double r_end = hit ? h.range : q.free_on_miss;
  const double dn = norm3(dir);
  const double dx = dir[0] / dn, dy = dir[1] / dn, dz = dir[2] / dn;
  int hcx = -8, hcy = -8;  // the hit's cell (-8: none, or outside the grid)
  if (hit) {
    const int cx = occ_cell(o[0] + h.range * dx, q.x0, q.res, q.nx);
    const int cy = occ_cell(o[1] + h.range * dy, q.y0, q.res, q.ny);
    if (cx >= 0 && cx < q.nx && cy >= 0 && cy < q.ny) hcx = cx, hcy = cy;
  }
  const bool silent = (q.flags & 1) && (h.flags & kRayOccupied);
  int ref = ter_q(o[2] - q.sensor_height, q.z_res);
  bool pending = false;  // a free piece lies in the hit's own cell
  // the walk: the ray's interval cut to the grid grown by a cell
  double ta = q.ray.t_min > 0.0 ? q.ray.t_min : 0.0, tb = r_end;
  bool walk = ta < tb;
  walk = walk && occ_clip(o[0], dx, q.x0 - q.res, q.x0 + (double)(q.nx + 1) * q.res, ta, tb);
  walk = walk && occ_clip(o[1], dy, q.y0 - q.res, q.y0 + (double)(q.ny + 1) * q.res, ta, tb);
  walk = walk && ta < tb;
  if (walk) {
    const int sx = dx > 0.0 ? 1 : (dx < 0.0 ? -1 : 0), sy = dy > 0.0 ? 1 : (dy < 0.0 ? -1 : 0);
    int kx = occ_cell(o[0] + ta * dx, q.x0, q.res, q.nx), ky = occ_cell(o[1] + ta * dy, q.y0, q.res, q.ny);
    double tnx = sx ? (((double)(kx + (sx > 0 ? 1 : 0)) * q.res + q.x0) - o[0]) / dx : __builtin_huge_val();
    double tny = sy ? (((double)(ky + (sy > 0 ? 1 : 0)) * q.res + q.y0) - o[1]) / dy : __builtin_huge_val();
    double t_in = ta;
    for (int step = q.nx + q.ny + 16; step > 0; step--) {  // (the cut bounds the walk; the count only backs it)
      const bool along_y = tny < tnx;
      const double t_exit = along_y ? tny : tnx;
      const double t_out = t_exit < tb ? t_exit : tb;
      if (t_out > t_in && kx >= 0 && kx < q.nx && ky >= 0 && ky < q.ny) {
        const size_t i = (size_t)ky * q.nx + kx;
        const int e = elev[i];
        if (e != kTerNone) ref = e;
        if (!silent && ter_band(q, ter_q(o[2] + 0.5 * (t_in + t_out) * dz, q.z_res), ref)) {
          if (kx == hcx && ky == hcy) pending = true;
          else atomicAdd(&n_free[i], 1);
        }
      }
      if (!(t_exit < tb)) break;  // (both axes still: t_exit = +inf, the one cell was judged)
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
  // the hit, against its own cell's elevation or the last ground the ray passed over
  if (hit) {
    const size_t i = (size_t)(hcy >= 0 ? hcy : 0) * q.nx + (hcx >= 0 ? hcx : 0);
    if (hcx >= 0) {
      const int e = elev[i];
      if (e != kTerNone) ref = e;
    }
    in_band = ter_band(q, ter_q(o[2] + h.range * dz, q.z_res), ref);
    if (hcx >= 0) {
      if (in_band) atomicAdd(&n_occ[i], 1);
      else if (pending) atomicAdd(&n_free[i], 1);
    }
  }
}

}  // namespace vg
