// vg_info.h — the expected pose information of rays against the map
// (vina_gpu.h "Localisability"): the per-ray term shared by k_info_places and
// k_info_scan (localizability.hip), the workgroup's fixed-order reduction of the
// 22 sums, and the record's finish (Schur complements, eig3). Reads the map only,
// through the traversal of vg_ray.h and the per-point body of vg_diff.h.
//
// The term. A ray from o along the unit d with the hit m at range r, n =
// m.normal, c = |m.ndotd|: J = [n ; (r d) x n] is the derivative of the residual
// n.(h - centre), h = o + r d, under o -> o + dp and d -> Exp(dtheta) d (unknowns
// [dp, dtheta], world frame, rotation about o: h moves by dp + dtheta x (r d)),
// s2 = c^2 (m.var + dept^2 + r^2 beam_dv (1 - c^2) / c^2) + floor_var — the
// bracket is diff_point's gate^2 / gate_sigma^2, the same operands in the same
// order — and the ray adds w J J^T, w = 1 / s2, entry (i, j) as (w J_i) J_j.
//
// The reduction. The 64 terms of a wave's lanes are added by a shuffle tree
// (offsets 32, 16, .. 1: lane l takes lane l + offset; a lane without a hit adds
// zeros), the tree's result goes into the wave's entry of 4 x 22 doubles of LDS
// (k_info_places: added to it, once per 256 directions, so that no sum lives in
// registers across a ray's walk), and the workgroup's first lane adds the four
// entries in wave order. Nothing else is shared, no atomics: the sums are a
// function of the terms and of which lane met them, nothing more.
#pragma once
#include "vg_diff.h"

namespace vg {

constexpr int kInfoBlock = kRayBlock;            // 256 threads, 4 waves
constexpr int kInfoWaves = kInfoBlock / 64;
constexpr int kInfoSums = 22;                    // H's upper triangle, row-major (sym_idx(6, i, j)), then sum_w
constexpr int kInfoEnded = kRayTruncated | kRayLeftRange;   // what sets VG_INFO_RAY_ENDED

struct InfoPrm {  // vg_info_params with the defaults applied
  RayPrm ray;
  double floor_var;
  int min_hits, pad;
};
inline InfoPrm info_prm(const vg_info_params* p) {
  InfoPrm q;
  q.ray = ray_prm(p ? &p->ray : nullptr);
  q.floor_var = p ? p->floor_var : 0.0;
  q.min_hits = p && p->min_hits > 0 ? p->min_hits : 16;
  q.pad = 0;
  return q;
}

struct InfoPart {  // a workgroup's sums (k_info_scan -> k_info_scan_sum), 184 bytes
  double s[kInfoSums];
  int n_hits, flags;
};

// rd: r d; r: the range of the beam-noise term (the hit's for a cast ray, the measured one for a scan point);
// m: a hit. False: the ray contributes nothing (s2 not finite or not > 0)
__device__ __forceinline__ bool info_term(const V3& rd, double r, const vg_ray_hit& m, double dept2, double beam_dv,
                                          double floor_var, double* J, double& w) {
  const V3 n = ld_v3(m.normal);
  const double c2 = m.ndotd * m.ndotd, beam2 = r * r * beam_dv;
  const double s2 = c2 * (m.var + dept2 + beam2 * (1.0 - c2) / c2) + floor_var;
  if (!(s2 > 0.0) || !ray_finite(s2)) return false;
  const V3 x = cross3(rd, n);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    J[j] = n[j];
    J[3 + j] = x[j];
  }
  w = 1.0 / s2;
  return true;
}

// one ray's 22 terms: entry (i, j) of w J J^T as (w J_i) J_j, then w
__device__ __forceinline__ void info_set(double* s, const double* J, double w) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const double wj = w * J[i];
#pragma unroll
    for (int j = i; j < 6; j++) s[k++] = wj * J[j];
  }
  s[kInfoSums - 1] = w;
}

// the wave's sum of every lane's s, n_hits and flags, in lane 0. Every lane of the wave calls it
__device__ __forceinline__ void info_wave_sum(double* s, int& n_hits, int& flags) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < kInfoSums; k++) s[k] += __shfl_down(s[k], off, 64);
    n_hits += __shfl_down(n_hits, off, 64);
    flags |= __shfl_down(flags, off, 64);
  }
}

// red: one entry per wave, written by the waves' first lanes; thread 0 adds them in wave order into tot.
// Every thread of the workgroup calls it
__device__ __forceinline__ void info_block_sum(const InfoPart* red, InfoPart& tot) {
  __syncthreads();
  if (threadIdx.x == 0) {
    tot = red[0];
    for (int v = 1; v < kInfoWaves; v++) {
#pragma unroll
      for (int k = 0; k < kInfoSums; k++) tot.s[k] += red[v].s[k];
      tot.n_hits += red[v].n_hits;
      tot.flags |= red[v].flags;
    }
  }
}

// eigenvalues ascending; the smallest one's unit eigenvector, its largest-magnitude component positive
__device__ __forceinline__ void info_eig(const M3& S, double* eig, double* dir) {
  V3 w;
  M3 V;
  eig3(S, w, V);
  int k = 0;
  for (int j = 1; j < 3; j++)
    if (fabs(V(j, 0)) > fabs(V(k, 0))) k = j;
  const double sg = V(k, 0) < 0.0 ? -1.0 : 1.0;
  for (int j = 0; j < 3; j++) {
    eig[j] = w[j];
    dir[j] = sg * V(j, 0);
  }
}

__device__ __forceinline__ bool info_degenerate(const M3& A) {
  V3 w;
  M3 V;
  eig3(A, w, V);
  return w[0] <= 1e-12 * w[2];
}

// s: the 22 sums; ended: some ray carried kInfoEnded. One thread writes the whole record
__device__ __forceinline__ void info_finish(const double* s, int n_rays, int n_hits, bool ended, int min_hits,
                                   vg_info_rec& out) {
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) out.H[6 * i + j] = s[sym_idx(6, i, j)];
  for (int j = 0; j < 3; j++) out.eig_t[j] = out.eig_r[j] = out.dir_t[j] = out.dir_r[j] = 0.0;
  out.sum_w = s[kInfoSums - 1];
  out.reserved = 0.0;
  out.n_rays = n_rays;
  out.n_hits = n_hits;
  out.pad = 0;
  int flags = ended ? VG_INFO_RAY_ENDED : 0;
  if (n_hits >= min_hits) {
    flags |= VG_INFO_VALID;
    M3 Hpp, Hpt, Htt;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        Hpp(i, j) = out.H[6 * i + j];
        Hpt(i, j) = out.H[6 * i + 3 + j];
        Htt(i, j) = out.H[6 * (3 + i) + 3 + j];
      }
    const bool deg_r = info_degenerate(Htt), deg_t = info_degenerate(Hpp);
    if (deg_r) flags |= VG_INFO_ROT_DEGENERATE;
    if (deg_t) flags |= VG_INFO_TRANS_DEGENERATE;
    if (deg_r) {
      info_eig(Hpp, out.eig_t, out.dir_t);
    } else if (deg_t) {
      info_eig(Htt, out.eig_r, out.dir_r);
    } else {
      const M3 Htp = tr(Hpt);
      info_eig(sub(Hpp, mul(mul(Hpt, inverse(Htt)), Htp)), out.eig_t, out.dir_t);
      info_eig(sub(Htt, mul(mul(Htp, inverse(Hpp)), Hpt)), out.eig_r, out.dir_r);
    }
  }
  out.flags = flags;
}

}  // namespace vg
