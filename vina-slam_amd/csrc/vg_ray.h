// vg_ray.h — a ray through the voxel map to the first plane it meets
// (vina_gpu.h "Ray-casting the map"; raycast.hip's kernels). Reads the DevMap
// the IEKF reads and writes nothing.
//
// A hit. A leaf L (NodeHdr::octo == 0, reachable from a hashed root) is a
// candidate of the ray (o, d, (t_lo, t_hi]) when is_plane is set, |n.d| >=
// min_cos with n, c its PlaneRec's, and h = o + t d with t = n.(c - o) / (n.d)
// has t in the interval and lies in L's cube under inside() (vg_match.h). The
// ray's hit is the candidate of smallest t, equal t to the lower node id.
//
// Traversal. Root cells (cell k spans [k vs, (k + 1) vs] per axis) are walked
// by Amanatides-Woo in double; a cell's exit is ((k + 1 | k) vs - o) / d of
// the axis, taken from the lattice plane itself and never accumulated, and
// its root is looked up by the packed integer key (not pack_key: that is the
// float rule of points). Inside a root the leaves are visited in the order of
// t without a stack: t_cur is the end of the last visited segment, and a
// descent from the root narrows [a, b) around t_cur at every internal node by
// its three centre-plane crossings s_j = (c_j - o_j) / d_j — a = max(a, the
// s_j <= t_cur), b = min(b, the s_j > t_cur) — and takes the child on the side
// of each centre plane the ray is on after (s_j <= t_cur) or before its
// crossing (the octant of any point of the open segment, its midpoint
// included, without rounding). Every value compared with t_cur is recomputed
// from the same operands each time, so the comparisons are exact, b > t_cur
// at every level, and t_cur strictly grows: no epsilon. At most 8 levels, as
// descend(). Segments that start past the best hit are not visited (a hit on
// a shared face, t == the segment's end, still lets the next leaf claim it).
//
// An axis with d_j = 0 has no crossing: the ray keeps o_j's side. Where o_j
// lies exactly on a lattice plane or on a node's centre plane the ray runs in
// the face shared by the cubes on both sides, and the inclusive cube test
// makes the leaves of both sides candidates. Such a tie is noticed where it
// is met, and the walk is then repeated with that axis' ties taken to the
// other side (at most 4 walks: a ray has at most two such axes); a ray that
// meets no tie, every ray with three non-zero components among them, is
// walked once.
//
// Every header read and every cell counts against max_steps, over all the
// walks of a ray; a ray that reaches it ends as a miss with kRayTruncated. No
// LDS, no atomics, no private array: a ray's record is a function of the ray
// and the map alone.
#pragma once
#include "vg_match.h"

namespace vg {

enum { kRayHit = 1, kRayTruncated = 2, kRayOccupied = 4, kRayLeftRange = 8, kRayInvalid = 16 };

struct RayPrm {  // vg_ray_params with the defaults applied
  double t_min, t_max, min_cos;
  int max_steps, pad;
};

__device__ __forceinline__ bool ray_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }

// the leaf's candidate; true when it beats (bt, bl)
__device__ __forceinline__ bool ray_leaf(const NodeHdr& h, const PlaneRec& P, int node, const V3& o, const V3& d,
                                         double t_lo, double t_hi, double min_cos, double& bt, int& bl, double& bnd) {
  const V3 n = ld_v3(P.normal), c = ld_v3(P.center);
  const double nd = dot3(n, d);
  if (!(fabs(nd) >= min_cos)) return false;
  const double t = dot3(n, sub(c, o)) / nd;
  if (!(t > t_lo && t <= t_hi)) return false;
  const V3 hp = v3(o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]);
  if (!inside(h, hp)) return false;
  if (bl >= 0 && !(t < bt || (t == bt && node < bl))) return false;
  bt = t;
  bl = node;
  bnd = nd;
  return true;
}

// the hit's record fields (the variance: match_leaf's first term over n.d squared)
__device__ __forceinline__ void ray_fill(const PlaneRec& P, const V3& o, const V3& d, double t, double nd,
                                         vg_ray_hit& out) {
  const V3 n = ld_v3(P.normal), c = ld_v3(P.center);
  const double J[6] = {o[0] + t * d[0] - c[0], o[1] + t * d[1] - c[1], o[2] + t * d[2] - c[2], -n[0], -n[1], -n[2]};
  double sl = 0.0;
  for (int j = 0; j < 6; j++) {
    double s = J[0] * P.var[sym_idx(6, 0, j)];
    for (int k = 1; k < 6; k++) s += J[k] * P.var[sym_idx(6, k, j)];
    sl = j == 0 ? s * J[0] : sl + s * J[j];
  }
  out.range = t;
  out.var = sl / (nd * nd);
  for (int j = 0; j < 3; j++) out.normal[j] = n[j];
  out.ndotd = nd;
}

// the walk's state that outlives one walk of the ray
struct RayAcc {
  double bt, bnd;  // the best candidate's t and n.d
  int bl;          // its leaf, -1: none
  int flags, steps;
  int ties;        // bit j: a tie on axis j (d_j = 0, o_j on a lattice or centre plane) was met
};

// One walk of the unit ray (o, d) over (t_lo, t_hi]. low: bit j takes axis j's
// ties to the lower side (else the upper). Returns false when the ray ended
// for good (step budget, key range).
__device__ __forceinline__ bool ray_walk(const DevMap& m, double vs, const V3& o, const V3& d, double t_lo, double t_hi,
                                         const RayPrm& prm, int low, RayAcc& A) {
  // the cell of the walk's first point; per axis the step and the exit's t
  // (scalars and unrolled selects: nothing here is indexed at run time)
  long long k[3];
  int stp[3];
  double t_next[3];
  bool in_range = true;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    stp[j] = d[j] > 0.0 ? 1 : (d[j] < 0.0 ? -1 : 0);
    double q = floor((o[j] + t_lo * d[j]) / vs);
    if (!stp[j] && q * vs == o[j]) {  // the ray runs in the lattice plane between the cells q - 1 and q
      A.ties |= 1 << j;
      if ((low >> j) & 1) q -= 1.0;
    }
    in_range = in_range && q >= -(double)kKeyOff && q < (double)kKeyOff;
    k[j] = in_range ? (long long)q : 0;
    t_next[j] = stp[j] ? ((double)(k[j] + (stp[j] > 0 ? 1 : 0)) * vs - o[j]) / d[j] : __builtin_huge_val();
  }
  if (!in_range) {
    if (A.bl < 0) A.flags |= kRayLeftRange;
    return false;
  }
  double t_in = t_lo;
  while (t_in < t_hi) {
    if (A.steps >= prm.max_steps) {
      A.flags |= kRayTruncated;
      return false;
    }
    A.steps++;
    // the axis the ray leaves this cell through (ties: the lowest axis)
    int ax = 0;
    double t_exit = t_next[0];
    if (t_next[1] < t_exit) ax = 1, t_exit = t_next[1];
    if (t_next[2] < t_exit) ax = 2, t_exit = t_next[2];
    const double t_out = t_exit < t_hi ? t_exit : t_hi;
    if (t_out > t_in) {
      const uint64_t key = ((uint64_t)(k[0] + kKeyOff) << 42) | ((uint64_t)(k[1] + kKeyOff) << 21) |
                           (uint64_t)(k[2] + kKeyOff);
      const int root = hash_find(m.hkey, m.hval, m.hash_mask, key);
      if (root >= 0 && root < m.cap_nodes) {
        double t_cur = t_in;
        while (t_cur < t_out && !(A.bl >= 0 && t_cur > A.bt)) {
          double a = t_in, b = t_out;
          int node = root;
          for (int depth = 0; depth < 8 && node >= 0; depth++) {
            if (A.steps >= prm.max_steps) {
              A.flags |= kRayTruncated;
              return false;
            }
            A.steps++;
            const NodeHdr& h = m.hdr[node];
            if (h.octo == 0) {
              if (h.is_plane) ray_leaf(h, m.pl[node], node, o, d, t_lo, t_hi, prm.min_cos, A.bt, A.bl, A.bnd);
              else if (h.last_num > 0 || h.fix_cnt > 0) A.flags |= kRayOccupied;
              break;
            }
            int oct = 0;
#pragma unroll
            for (int j = 0; j < 3; j++) {
              bool up;
              if (stp[j]) {
                const double s = (h.center[j] - o[j]) / d[j];
                const bool passed = s <= t_cur;
                if (passed) a = s > a ? s : a;
                else b = s < b ? s : b;
                up = passed == (stp[j] > 0);
              } else {
                up = o[j] > h.center[j];
                if (o[j] == h.center[j]) {  // the ray runs in this centre plane
                  A.ties |= 1 << j;
                  up = !((low >> j) & 1);
                }
              }
              oct = 2 * oct + (up ? 1 : 0);
            }
            const int ch = h.child[oct];
            node = (ch >= 0 && ch < m.cap_nodes) ? ch : -1;
          }
          t_cur = b;  // b > t_cur at every level: the walk advances
        }
      }
    }
    if (A.bl >= 0 && t_exit > A.bt) break;  // the next cell starts past the hit
    // into the next cell
    t_in = t_exit > t_in ? t_exit : t_in;
    bool left = false;
#pragma unroll
    for (int j = 0; j < 3; j++)
      if (j == ax) {
        k[j] += stp[j];
        left = k[j] < -kKeyOff || k[j] >= kKeyOff;
        t_next[j] = ((double)(k[j] + (stp[j] > 0 ? 1 : 0)) * vs - o[j]) / d[j];
      }
    if (left) {
      if (t_in < t_hi && A.bl < 0) A.flags |= kRayLeftRange;
      return false;
    }
  }
  return true;
}

// o: origin, dir: direction (any length); the record is complete on return
__device__ __forceinline__ void ray_trace(const DevMap& m, double vs, const V3& o, const V3& dir, const RayPrm& prm,
                                          vg_ray_hit& out) {
  out.range = 0.0;
  out.var = 0.0;
  out.normal[0] = out.normal[1] = out.normal[2] = 0.0;
  out.ndotd = 0.0;
  out.leaf = -1;
  out.flags = 0;
  out.reserved = 0.0;
  const double dn = norm3(dir);
  if (!(dn > 0.0) || !ray_finite(dn) || !ray_finite(o[0]) || !ray_finite(o[1]) || !ray_finite(o[2])) {
    out.flags = kRayInvalid;  // (a NaN fails dn > 0 or the finite tests)
    return;
  }
  const V3 d = v3(dir[0] / dn, dir[1] / dn, dir[2] / dn);
  const double t_lo = prm.t_min > 0.0 ? prm.t_min : 0.0, t_hi = prm.t_max;
  RayAcc A;
  A.bt = A.bnd = 0.0;
  A.bl = -1;
  A.flags = A.steps = A.ties = 0;
  // the walk with every tie taken up, then one per non-empty set of the axes on which a tie was met
  for (int low = 0; low < 8; low++) {
    if ((low & A.ties) != low) continue;
    if (!ray_walk(m, vs, o, d, t_lo, t_hi, prm, low, A)) break;
  }
  if (A.bl >= 0 && !(A.flags & kRayTruncated)) {
    ray_fill(m.pl[A.bl], o, d, A.bt, A.bnd, out);
    out.leaf = A.bl;
    A.flags |= kRayHit;
  }
  out.flags = A.flags;
#ifdef VG_PROBE
  out.reserved = (double)A.steps;  // cells + nodes visited (scripts/probe_raycast.py)
#endif
}

}  // namespace vg
