// vg_match.h — the correspondence rule of OctoTree::match (octree.cpp:551-595,
// voxel_map.cpp:241-266) and the halving wave sums, shared by the IEKF point
// loop (iekf.hip) and the pose-hypothesis scoring (score.hip): the descent from
// a root voxel, the probabilistic point-to-plane gate at a leaf, the matched
// point's contribution to the normal equations, and the butterfly both
// reductions are built from.
#pragma once
#include "vg_iekf.h"

namespace vg {

__device__ __forceinline__ int descend(const NodeHdr* __restrict__ hdr, int node, const V3& w) {
  for (int d = 0; d < 8 && node >= 0; d++) {
    const NodeHdr& h = hdr[node];
    if (h.octo == 0) return node;
    node = h.child[octant(w, h.center)];
  }
  return -1;
}

// OctoTree::match at a leaf; returns 1 and sigma on success
__device__ __forceinline__ int match_leaf(const NodeHdr& h, const PlaneRec& P, const V3& wld, const M3& var_wld,
                                          double& sigma) {
  if (!h.is_plane) return 0;
  V3 c = ld_v3(P.center), n = ld_v3(P.normal);
  V3 d = sub(wld, c);
  float dis_to_plane = fabs(dot3(n, d));
  V3 cw = sub(c, wld);
  float dis_to_center = cw[0] * cw[0] + cw[1] * cw[1] + cw[2] * cw[2];
  float range_dis = (dis_to_center - dis_to_plane * dis_to_plane);
  if (!(range_dis <= 3 * 3 * P.radius)) return 0;
  double J[6] = {d[0], d[1], d[2], -n[0], -n[1], -n[2]};
  double t[6];
  for (int j = 0; j < 6; j++) {
    double s = J[0] * P.var[sym_idx(6, 0, j)];
    for (int k = 1; k < 6; k++) s += J[k] * P.var[sym_idx(6, k, j)];
    t[j] = s;
  }
  double sl = t[0] * J[0];
  for (int j = 1; j < 6; j++) sl += t[j] * J[j];
  V3 vn = mul(var_wld, n);
  sl += dot3(n, vn);
  if (dis_to_plane < 3 * sqrt(sl)) {
    sigma = sl;
    return 1;
  }
  return 0;
}

__device__ __forceinline__ bool inside(const NodeHdr& h, const V3& w) {
  double hl = h.qlen * 2;
  return (w[0] >= h.center[0] - hl && w[0] <= h.center[0] + hl && w[1] >= h.center[1] - hl &&
          w[1] <= h.center[1] + hl && w[2] >= h.center[2] - hl && w[2] <= h.center[2] + hl);
}

// A matched point's terms of the weighted normal equations (odometry.cpp:133-147)
// added to the 34 sums: HTH (upper 21), HTz (6), nnt (upper 6), the match count.
// pnt: the body point, Rt: the pose's rotation transposed, wld: the world point,
// P: the matched leaf's plane, sigma: match_leaf's
__device__ __forceinline__ void iekf_accum(double (&acc)[kIekfVals], const PlaneRec& P, const V3& pnt, const M3& Rt,
                                           const V3& wld, double sigma) {
  V3 nn = ld_v3(P.normal), c = ld_v3(P.center);
  double R_inv = 1.0 / (0.0005 + sigma);
  double resi = dot3(nn, sub(wld, c));
  V3 j3 = mul(mul(hat(pnt), Rt), nn);
  double jac[6] = {j3[0], j3[1], j3[2], nn[0], nn[1], nn[2]};
  int k = 0;
  for (int r = 0; r < 6; r++) {
    double jr_ = jac[r] * R_inv;
    for (int c2 = r; c2 < 6; c2++, k++) acc[k] += jr_ * jac[c2];
  }
  for (int r = 0; r < 6; r++) acc[21 + r] -= jac[r] * (R_inv * resi);
  acc[27] += nn[0] * nn[0];
  acc[28] += nn[0] * nn[1];
  acc[29] += nn[0] * nn[2];
  acc[30] += nn[1] * nn[1];
  acc[31] += nn[1] * nn[2];
  acc[32] += nn[2] * nn[2];
  acc[33] += 1.0;
}

// ---- wave sums without LDS: the partner across lane bit L (lane ^ L) via
// gfx950's v_permlane32_swap / v_permlane16_swap and DPP (row_ror:8, row
// shifts by 4, quad perms)
__device__ __forceinline__ double pack_d(unsigned lo, unsigned hi) {
  return __longlong_as_double(((long long)hi << 32) | lo);
}
template <int C>
__device__ __forceinline__ unsigned dpp32(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, C, 0xf, 0xf, false);
}
template <int L>
__device__ __forceinline__ double xor_lane(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
  if constexpr (L == 32) {  // r[0] = x[lane % 32], r[1] = x[lane % 32 + 32]
    auto l2 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto h2 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return (lane & 32) ? pack_d(l2[0], h2[0]) : pack_d(l2[1], h2[1]);
  } else if constexpr (L == 16) {  // r[0] = the even row's x, r[1] = the odd row's
    auto l2 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto h2 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return (lane & 16) ? pack_d(l2[0], h2[0]) : pack_d(l2[1], h2[1]);
  } else if constexpr (L == 8) {
    return pack_d(dpp32<0x128>(lo), dpp32<0x128>(hi));  // row_ror:8
  } else if constexpr (L == 4) {
    const double up = pack_d(dpp32<0x104>(lo), dpp32<0x104>(hi));  // row_shl:4 (lane i <- i + 4)
    const double dn = pack_d(dpp32<0x114>(lo), dpp32<0x114>(hi));  // row_shr:4 (lane i <- i - 4)
    return (lane & 4) ? dn : up;
  } else if constexpr (L == 2) {
    return pack_d(dpp32<0x4E>(lo), dpp32<0x4E>(hi));  // quad_perm [2,3,0,1]
  } else {
    return pack_d(dpp32<0xB1>(lo), dpp32<0xB1>(hi));  // quad_perm [1,0,3,2]
  }
}
// one level of a halving wave sum: the lanes with bit L clear keep the first
// ceil(N/2) values, the others the rest, each adding its partner's copy
template <int L, int N>
__device__ __forceinline__ void halve(const double (&v)[N], double (&w)[(N + 1) / 2], int lane, int& idx, int& n) {
  constexpr int H = (N + 1) / 2;
  const bool hi = (lane & L) != 0;
#pragma unroll
  for (int j = 0; j < H; j++) {
    const double a = v[j], b = (H + j < N) ? v[H + j] : 0.0;
    w[j] = (hi ? b : a) + xor_lane<L>(hi ? a : b, lane);
  }
  if (hi) {
    idx += H;
    n = n > H ? n - H : 0;
  } else {
    n = n < H ? n : H;
  }
}

// the workgroup's 34 sums (threads < 34 hold one each): a halving butterfly
// per wave, then LDS across the 4 waves (fixed tree). Every level pairs lane ^
// L for L = 32, 16, ..., 1, so each sum is bit for bit lane 0's of a shfl_down
// tree, but a lane hands over half of the values it carries at every level:
// 37 exchanges for the 34 sums instead of 204, through permlane / DPP
__device__ __forceinline__ double iekf_wg_sum(double (&acc)[kIekfVals], double (*red)[kIekfVals]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  static_assert(kIekfVals == 34, "the halving levels below are laid out for 34 sums");
  int ridx = 0, rn = kIekfVals;
  double h17[17], h9[9], h5[5], h3[3], h2[2], h1[1];
  halve<32>(acc, h17, lane, ridx, rn);
  halve<16>(h17, h9, lane, ridx, rn);
  halve<8>(h9, h5, lane, ridx, rn);
  halve<4>(h5, h3, lane, ridx, rn);
  halve<2>(h3, h2, lane, ridx, rn);
  halve<1>(h2, h1, lane, ridx, rn);
  if (rn == 1) red[wv][ridx] = h1[0];
  __syncthreads();
  const int j = threadIdx.x < kIekfVals ? threadIdx.x : 0;
  return ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
}

// ---- the IEKF point loop (iekf.hip k_iekf, fleet.hip k_fleet_iekf)
// The pose (x_curr R, p and the rotation / translation covariance blocks) is
// read from the device state the previous k_iekf_update wrote; the kernel is a
// no-op once the IEKF has finished (st->done). Iteration 0 ignores the leaf
// cache (no association yet, odometry.cpp:111-132).
// one IEKF iteration's point loop over the workgroup's chunk vb (k_iekf): the
// 34 sums of this lane's points
// kPf: a point whose cached leaf matched last iteration (octos[i]) touches its
// plane record's 128 B lines right away, beside the header load, so the
// gate's record reads hit in cache instead of a second dependent miss
template <bool kPf = false>
__device__ __forceinline__ void iekf_points(const MP& mp, const DState* __restrict__ st, const DevMap& m,
                                            int* __restrict__ cache, int* __restrict__ pk, int it, int nb, int vb,
                                            const M3& R, const V3& p, const M3& rot_var, const M3& tsl_var,
                                            double (&acc)[kIekfVals]) {
  const int* __restrict__ keep = iekf_keep(st);
  const int n = keep ? st->snk : st->sn;
  const float* __restrict__ x = st->sx;
  const float* __restrict__ y = st->sy;
  const float* __restrict__ z = st->sz;
  const M3 Rt = tr(R);
  for (int j = 0; j < kIekfVals; j++) acc[j] = 0.0;
  for (int q = vb * blockDim.x + threadIdx.x; q < n; q += nb * blockDim.x) {
    const int i = keep ? keep[q] : q;  // the raw index (the memo and the profiling pass are per raw point)
    V3 pnt;
    M3 var;
    var_init_pt(mp, x[i], y[i], z[i], pnt, var);
    M3 var_world = world_var(R, var, pnt, rot_var, tsl_var);
    V3 wld = rigid(R, pnt, p);
    // cache[i]: the leaf of the point's last match (the reference's octos[i],
    // odometry.cpp:124-131, reset per scan) or, after a failed match, the
    // leaf the descent reached — a memo only (bit 30 tags it): while the
    // point stays inside that leaf's box and its float voxel key still names
    // the leaf's root (the lookup rounds in float, voxel_map.cpp:246-253), the
    // lookup would reach the same leaf, so unmatched points skip the hash +
    // descent too
    const int cv = it > 0 ? cache[i] : -1;
    int leaf = cv >= 0 ? (cv & 0x3fffffff) : -1;
    int flag = 0;
    double sigma = 0;
    double pf0 = 0.0, pf1 = 0.0, pf2 = 0.0;
    if (kPf && cv >= 0 && !(cv & 0x40000000)) {  // bytes 0, 112, 216: every 128 B line the 224 B record spans
      const double* rec = reinterpret_cast<const double*>(&m.pl[leaf]);
      pf0 = rec[0];
      pf1 = rec[14];
      pf2 = rec[27];
    }
    // a matched leaf (octos[i]): OctoTree::inside's inclusive box; a memo: the
    // descent's own region (dbox: strict where the descent is strict), so a
    // point on a centre plane is never kept in the wrong sibling
    bool hit = leaf >= 0 && ((cv & 0x40000000) ? in_dbox(m.dbox + (size_t)leaf * 6, wld) : inside(m.hdr[leaf], wld));
    if (hit && (cv & 0x40000000)) {
      uint64_t kw, kl;
      const NodeHdr& hl = m.hdr[leaf];
      hit = pack_key(wld, mp.vs, kw) && pack_key(v3(hl.center[0], hl.center[1], hl.center[2]), mp.vs, kl) && kw == kl;
    }
    if (hit) {
      if (kPf) asm volatile("" ::"v"(pf0), "v"(pf1), "v"(pf2));  // the touches complete here, not before
      flag = match_leaf(m.hdr[leaf], m.pl[leaf], wld, var_world, sigma);
      if (!flag && !(cv & 0x40000000)) leaf = -2;  // the reference's octos[i] stays: keep the cache
    } else {
      leaf = -1;
      uint64_t key;
      if (pack_key(wld, mp.vs, key) && owns(m, key)) {  // another shard's tile: not matched here
        int root = hash_find(m.hkey, m.hval, m.hash_mask, key);
        int lf = root >= 0 ? descend(m.hdr, root, wld) : -1;
        if (lf >= 0) {
          flag = match_leaf(m.hdr[lf], m.pl[lf], wld, var_world, sigma);
          leaf = lf;
        }
      }
    }
    if (pk) pk[i] = flag ? leaf : -1;  // the leaf whose plane this iteration read (profiling pass)
    if (flag) {
      cache[i] = leaf;
    } else if (leaf >= 0) {
      if (it == 0 || cv < 0 || (cv & 0x40000000)) cache[i] = leaf | 0x40000000;  // no octos[i] to keep
    } else if (leaf == -1 && (it == 0 || cv < 0 || (cv & 0x40000000))) {
      cache[i] = -1;
    }
    if (flag) iekf_accum(acc, m.pl[leaf], pnt, Rt, wld, sigma);
  }
}
// (iekf_wg_sum, the workgroup's 34 sums: vg_match.h)
// the pose words an iteration's point loop reads from x_curr: R 9, p 3, the
// rotation and translation covariance blocks 9 + 9
__device__ __forceinline__ double pose_word(const double* xc, int t) {
  if (t < 12) return xc[t];
  if (t < 21) return xc[kXS + ((t - 12) / 3) * 15 + (t - 12) % 3];
  return xc[kXS + (3 + (t - 21) / 3) * 15 + 3 + (t - 21) % 3];
}
__device__ __forceinline__ void pose_of(const double* w, M3& R, V3& p, M3& rot_var, M3& tsl_var) {
  for (int q = 0; q < 9; q++) {
    R[q] = w[q];
    rot_var[q] = w[12 + q];
    tsl_var[q] = w[21 + q];
  }
  p = v3(w[9], w[10], w[11]);
}

}  // namespace vg
