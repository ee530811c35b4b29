// vg_place.h — the place index's descriptor (vina_gpu.h "Place index"): a
// gravity-aligned polar range image of A azimuth x E elevation bins, one
// uint16 per bin (range in 1 / 512 m, 0: none), shared by the host
// (places_host.cpp: the direction table, the defaults) and by the kernels
// (places.hip: a scan point's bin).
//
// The frame is (ex, ey, up): up = -g / |g| of the context's state, ex = world x
// made perpendicular to up (world y where up is within 26 degrees of x), ey =
// up x ex. Azimuth bin a covers [a, a + 1) 2 pi / A from ex towards ey;
// elevation bin e covers el_min + [e, e + 1) (el_max - el_min) / E. The map
// side casts one ray per bin through the bin's centre; the scan side takes the
// mean range of the points that fall into the bin. A circular shift of the
// azimuth axis by s bins is a yaw of 2 pi s / A about up, which is what the
// match searches. Everything after a ray's range or a point's (bin, range) is
// integer arithmetic.
#pragma once
#include "vg_diff.h"

namespace vg {

constexpr int kPlaceMaxAz = 256, kPlaceMaxEl = 32, kPlaceMaxBins = 4096;
constexpr double kPlaceQ = 512.0;  // quantisation steps per metre
constexpr int kPlaceBlock = 256;
constexpr double kTwoPi = 6.283185307179586476925286766559;

struct PlacePrm {  // vg_places_params with the defaults applied
  int n_az, n_el, min_bins, clip_q;
  double el_min, el_max, t_max;
  RayPrm ray;  // t_max: the one above
};

// false: a limit is exceeded or a span is empty
inline bool place_prm(const vg_places_params* p, PlacePrm& q) {
  q.n_az = p && p->n_az > 0 ? p->n_az : 120;
  q.n_el = p && p->n_el > 0 ? p->n_el : 12;
  const bool span = p && (p->el_min != 0.0 || p->el_max != 0.0);
  q.el_min = span ? p->el_min : -kTwoPi / 12.0;
  q.el_max = span ? p->el_max : kTwoPi / 12.0;
  q.t_max = p && p->t_max > 0.0 ? p->t_max : 60.0;
  const double clip = p && p->clip > 0.0 ? p->clip : 2.0;
  if (q.n_az > kPlaceMaxAz || q.n_el > kPlaceMaxEl || q.n_az * q.n_el > kPlaceMaxBins) return false;
  if (!(q.el_min < q.el_max) || !(q.el_min >= -kTwoPi / 4.0) || !(q.el_max <= kTwoPi / 4.0)) return false;
  if (!(q.t_max <= 1e6) || !(clip <= 1e6)) return false;
  const double cq = rint(clip * kPlaceQ);
  q.clip_q = cq > 65535.0 ? 65535 : (int)cq;
  q.min_bins = p && p->min_bins > 0 ? p->min_bins : (q.n_az * q.n_el / 8 > 0 ? q.n_az * q.n_el / 8 : 1);
  q.ray = ray_prm(p ? &p->ray : nullptr);
  q.ray.t_max = q.t_max;
  return true;
}

// bin e * A + a's centre direction in the descriptor's own frame (x, y, up)
inline void place_dir(const PlacePrm& q, int e, int a, double* d) {
  const double el = q.el_min + (e + 0.5) * ((q.el_max - q.el_min) / q.n_el);
  const double az = (a + 0.5) * (kTwoPi / q.n_az);
  d[0] = cos(el) * cos(az);
  d[1] = cos(el) * sin(az);
  d[2] = sin(el);
}

// a range in metres as a bin's value
__host__ __device__ inline unsigned place_quant(double r) {
  const double q = rint(r * kPlaceQ);
  return q > 65535.0 ? 65535u : (q > 0.0 ? (unsigned)q : 0u);
}

struct PlaceFrame {  // rows ex, ey, up; M = R_level ext_R
  double f[9], m[9];
};

// A scan point x (LiDAR frame): its bin, or -1 when it is dropped (outside the
// elevation span, beyond t_max, at the origin), and q = rint(512 |v|)
__device__ __forceinline__ int place_bin(const PlacePrm& p, const PlaceFrame& F, double x0, double x1, double x2,
                                         unsigned& q) {
  const double v0 = F.m[0] * x0 + F.m[1] * x1 + F.m[2] * x2;
  const double v1 = F.m[3] * x0 + F.m[4] * x1 + F.m[5] * x2;
  const double v2 = F.m[6] * x0 + F.m[7] * x1 + F.m[8] * x2;
  const double r = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  if (!(r > 0.0) || !(r <= p.t_max)) return -1;
  const double cx = F.f[0] * v0 + F.f[1] * v1 + F.f[2] * v2;
  const double cy = F.f[3] * v0 + F.f[4] * v1 + F.f[5] * v2;
  const double cz = F.f[6] * v0 + F.f[7] * v1 + F.f[8] * v2;
  double az = atan2(cy, cx);
  if (az < 0.0) az += kTwoPi;
  const double el = asin(cz / r);
  const double fe = floor((el - p.el_min) / ((p.el_max - p.el_min) / p.n_el));
  if (!(fe >= 0.0) || !(fe < (double)p.n_el)) return -1;
  double fa = floor(az / (kTwoPi / p.n_az));
  if (!(fa >= 0.0)) return -1;  // (a NaN)
  if (fa > (double)(p.n_az - 1)) fa = (double)(p.n_az - 1);
  const double qq = rint(r * kPlaceQ);
  q = qq > 65535.0 ? 65535u : (unsigned)qq;
  return (int)fe * p.n_az + (int)fa;
}

}  // namespace vg
