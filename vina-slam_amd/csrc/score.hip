// score.hip — pose-hypothesis scoring: the matching rule of OctoTree::match
// (octree.cpp:551-595, voxel_map.cpp:241-266) for one scan under many candidate
// poses in one dispatch (vg_score_poses), and the IEKF's 6 x 6 normal
// equations of a cloud at one given pose (vg_relocalize's Gauss-Newton).
// Both read the map only and share the IEKF's device functions (vg_match.h,
// vg_dev.h); there is no per-scan memo cache here, which is per scan and pose.
//
// k_score: a 2-D grid of point chunks (x, 256 points, one per lane) by pose
// tiles (y, kScoreTile poses). A lane computes its point's var_init once, then
// loops over the tile: rigid transform, voxel key, root lookup, descent, and at
// a leaf the world covariance and the gate. The only locality the kernel has is
// the L2: the caller orders the poses so that a tile's 16 are neighbours in its
// search grid (vg_reloc_grid: 4 x 4 patches of the x-y plane), and a
// workgroup's 256 consecutive points then walk the same root voxels and plane
// records 16 times over.
//
// Reduction: per pose a halving butterfly per wave (vg_match.h), the four
// waves' sums added in wave order, the workgroup's kScoreVals partials stored
// to HBM at [chunk][pose]; k_score_sum adds each pose's chunks in chunk order.
// No floating-point atomics; the chunking depends on n only and a pose's sums
// on nothing but its own chunks, so a pose's record has the same bits scored
// alone or at any position of any batch. The host walks K in slabs sized to
// the partials' scratch (one launch for K = 4,096 on a 10^4-point cloud).
#include "vg_match.h"

namespace vg {

constexpr int kScoreVals = 10;  // matches, in_map, cost, sum |r|, nn upper 6
constexpr int kScoreTile = 16;  // poses per workgroup
constexpr int kScoreChunk = 256;
constexpr size_t kScorePartBytes = size_t(1) << 26;  // the partials' scratch a slab may take

struct PoseVar {
  double v[18];  // rot_var 3x3, tsl_var 3x3
};

// the point's root voxel and leaf at pose (R, p); returns the match flag
__device__ __forceinline__ int score_point(const MP& mp, const DevMap& m, const V3& pnt, const M3& var, const M3& R,
                                           const V3& p, const M3& rot_var, const M3& tsl_var, V3& wld, int& leaf,
                                           double& sigma) {
  wld = rigid(R, pnt, p);
  leaf = -1;
  sigma = 0.0;
  uint64_t key;
  if (!pack_key(wld, mp.vs, key)) return 0;  // out of the packed range: not in the map
  const int root = hash_find(m.hkey, m.hval, m.hash_mask, key);
  const int lf = root >= 0 ? descend(m.hdr, root, wld) : -1;
  if (lf < 0) return 0;
  leaf = lf;
  const M3 var_world = world_var(R, var, pnt, rot_var, tsl_var);
  return match_leaf(m.hdr[lf], m.pl[lf], wld, var_world, sigma);
}

// partials: [chunk][kn poses][kScoreVals] for the poses [k0, k0 + kn)
__global__ void __launch_bounds__(kScoreChunk) k_score(MP mp, DevMap m, const float* __restrict__ xyz, int n,
                                                       const double* __restrict__ poses, int k0, int kn, PoseVar pv,
                                                       double* __restrict__ partials,
                                                       vg_point_match* __restrict__ pp) {
  __shared__ double s_pose[kScoreTile][12];
  __shared__ double red[kScoreTile][4][kScoreVals];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int q0 = blockIdx.y * kScoreTile;
  const int tn = kn - q0 < kScoreTile ? kn - q0 : kScoreTile;
  for (int e = tid; e < tn * 12; e += kScoreChunk) s_pose[e / 12][e % 12] = poses[(size_t)(k0 + q0 + e / 12) * 12 + e % 12];
  const int i = blockIdx.x * kScoreChunk + tid;
  const bool valid = i < n;
  V3 pnt = v3(0, 0, 1);
  M3 var = M3::Z();
  if (valid) var_init_pt(mp, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], pnt, var);
  M3 rot_var, tsl_var;
  for (int e = 0; e < 9; e++) {
    rot_var[e] = pv.v[e];
    tsl_var[e] = pv.v[9 + e];
  }
  __syncthreads();
  for (int t = 0; t < tn; t++) {
    double acc[kScoreVals];
    for (int j = 0; j < kScoreVals; j++) acc[j] = 0.0;
    if (valid) {
      const M3 R = ld_m3(s_pose[t]);
      const V3 p = ld_v3(s_pose[t] + 9);
      V3 wld;
      int leaf;
      double sigma;
      const int flag = score_point(mp, m, pnt, var, R, p, rot_var, tsl_var, wld, leaf, sigma);
      double r = 0.0;
      if (leaf >= 0) acc[1] = 1.0;
      if (flag) {
        const PlaneRec& P = m.pl[leaf];
        const V3 nn = ld_v3(P.normal);
        r = dot3(nn, sub(wld, ld_v3(P.center)));
        acc[0] = 1.0;
        acc[2] = r * r / (0.0005 + sigma);
        acc[3] = fabs(r);
        acc[4] = nn[0] * nn[0];
        acc[5] = nn[0] * nn[1];
        acc[6] = nn[0] * nn[2];
        acc[7] = nn[1] * nn[1];
        acc[8] = nn[1] * nn[2];
        acc[9] = nn[2] * nn[2];
      }
      if (pp) {  // (K = 1)
        vg_point_match o;
        o.leaf = leaf;
        o.flag = flag;
        o.r = r;
        o.sigma_d = flag ? sigma : 0.0;
        pp[i] = o;
      }
    }
    int ridx = 0, rn = kScoreVals;
    double h5[5], h3[3], h2[2], h1[1], g1[1], f1[1];
    halve<32>(acc, h5, lane, ridx, rn);
    halve<16>(h5, h3, lane, ridx, rn);
    halve<8>(h3, h2, lane, ridx, rn);
    halve<4>(h2, h1, lane, ridx, rn);
    halve<2>(h1, g1, lane, ridx, rn);
    halve<1>(g1, f1, lane, ridx, rn);
    if (rn == 1) red[t][wv][ridx] = f1[0];
  }
  __syncthreads();
  for (int e = tid; e < tn * kScoreVals; e += kScoreChunk) {
    const int t = e / kScoreVals, j = e % kScoreVals;
    partials[((size_t)blockIdx.x * kn + q0 + t) * kScoreVals + j] = ((red[t][0][j] + red[t][1][j]) + red[t][2][j]) + red[t][3][j];
  }
}

// each pose's chunks in chunk order -> its record
__global__ void __launch_bounds__(256) k_score_sum(const double* __restrict__ partials, int nchunks, int k0, int kn,
                                                   vg_pose_score* __restrict__ out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= kn) return;
  double s[kScoreVals];
  for (int j = 0; j < kScoreVals; j++) s[j] = 0.0;
  for (int c = 0; c < nchunks; c++) {
    const double* pr = partials + ((size_t)c * kn + q) * kScoreVals;
    for (int j = 0; j < kScoreVals; j++) s[j] += pr[j];
  }
  vg_pose_score o;
  o.matches = (int)s[0];
  o.in_map = (int)s[1];
  o.cost = s[2];
  o.sum_abs = s[3];
  for (int j = 0; j < 6; j++) o.nn[j] = s[4 + j];
  o.reserved = 0.0;
  out[k0 + q] = o;
}

// The IEKF's sums (iekf_accum: HTH, HTz, nnt, the match count) of the cloud at
// one pose, a fresh association for every point: a workgroup per chunk, its 34
// partials at [chunk]
__global__ void __launch_bounds__(kScoreChunk) k_score_normal(MP mp, DevMap m, const float* __restrict__ xyz, int n,
                                                              PoseVar pose, PoseVar pv,
                                                              double* __restrict__ partials) {
  __shared__ double red[4][kIekfVals];
  const int i = blockIdx.x * kScoreChunk + threadIdx.x;
  double acc[kIekfVals];
  for (int j = 0; j < kIekfVals; j++) acc[j] = 0.0;
  if (i < n) {
    V3 pnt;
    M3 var, rot_var, tsl_var;
    var_init_pt(mp, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], pnt, var);
    for (int e = 0; e < 9; e++) {
      rot_var[e] = pv.v[e];
      tsl_var[e] = pv.v[9 + e];
    }
    const M3 R = ld_m3(pose.v);
    const V3 p = ld_v3(pose.v + 9);
    V3 wld;
    int leaf;
    double sigma;
    if (score_point(mp, m, pnt, var, R, p, rot_var, tsl_var, wld, leaf, sigma))
      iekf_accum(acc, m.pl[leaf], pnt, tr(R), wld, sigma);
  }
  const double v = iekf_wg_sum(acc, red);
  if (threadIdx.x < kIekfVals) partials[(size_t)blockIdx.x * kIekfVals + threadIdx.x] = v;
}
__global__ void __launch_bounds__(64) k_score_normal_sum(const double* __restrict__ partials, int nchunks,
                                                         double* __restrict__ out) {
  const int j = threadIdx.x;
  if (j >= kIekfVals) return;
  double s = 0.0;
  for (int c = 0; c < nchunks; c++) s += partials[(size_t)c * kIekfVals + j];
  out[j] = s;
}

// ---- host side

static PoseVar pose_var_arg(const double* pose_var) {
  PoseVar pv;
  for (int e = 0; e < 18; e++) pv.v[e] = pose_var ? pose_var[e] : 0.0;
  return pv;
}

static int score_upload(vg_ctx* ctx, const float* xyz, int n) {
  ScoreBufs& b = ctx->score;
  if (!xyz) return VG_OK;
  VG_HIP(b.xyz.reserve_pow2((size_t)(n > 0 ? n : 1) * 3));
  if (n > 0) VG_HIP(hipMemcpyAsync(b.xyz, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  b.n = n;
  return VG_OK;
}

int score_poses_dev(vg_ctx* ctx, const MP& mp, const float* xyz, int n, const double* poses, int K,
                    const double* pose_var, vg_pose_score* out, void* per_point) {
  ScoreBufs& b = ctx->score;
  hipStream_t s = ctx->stream;
  VG_TRY(score_upload(ctx, xyz, n));
  n = b.n;
  memset(out, 0, (size_t)K * sizeof(vg_pose_score));
  if (n <= 0) return VG_OK;
  const int nchunks = (n + kScoreChunk - 1) / kScoreChunk;
  // poses per launch: what the partials' scratch holds, whole tiles
  size_t slab = kScorePartBytes / ((size_t)nchunks * kScoreVals * sizeof(double));
  slab = slab / kScoreTile * kScoreTile;
  if (slab < (size_t)kScoreTile) slab = kScoreTile;
  if (slab > (size_t)K) slab = (size_t)K;
  VG_HIP(b.poses.reserve_pow2((size_t)K * 12));
  VG_HIP(b.partials.reserve_pow2((size_t)nchunks * slab * kScoreVals));
  VG_HIP(b.out.reserve_pow2((size_t)K));
  if (per_point) VG_HIP(b.pp.reserve_pow2((size_t)n));
  vg_pose_score* d_out = b.out;
  vg_point_match* d_pp = per_point ? b.pp.p : nullptr;
  VG_HIP(hipMemcpyAsync(b.poses, poses, (size_t)K * 12 * sizeof(double), hipMemcpyHostToDevice, s));
  const PoseVar pv = pose_var_arg(pose_var);
  VG_HIP(b.t.begin(s));
  for (int k0 = 0; k0 < K; k0 += (int)slab) {
    const int kn = K - k0 < (int)slab ? K - k0 : (int)slab;
    const dim3 grid(nchunks, (kn + kScoreTile - 1) / kScoreTile);
    k_score<<<grid, kScoreChunk, 0, s>>>(mp, ctx->map, b.xyz, n, b.poses, k0, kn, pv, b.partials, d_pp);
    k_score_sum<<<(kn + 255) / 256, 256, 0, s>>>(b.partials, nchunks, k0, kn, d_out);
  }
  VG_HIP(b.t.end(s));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(out, d_out, (size_t)K * sizeof(vg_pose_score), hipMemcpyDeviceToHost, s));
  if (per_point) VG_HIP(hipMemcpyAsync(per_point, d_pp, (size_t)n * sizeof(vg_point_match), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  return VG_OK;
}

int score_normal_dev(vg_ctx* ctx, const MP& mp, const double* pose12, const double* pose_var, double* out34) {
  ScoreBufs& b = ctx->score;
  hipStream_t s = ctx->stream;
  const int n = b.n;
  for (int j = 0; j < kIekfVals; j++) out34[j] = 0.0;
  if (n <= 0) return VG_OK;
  const int nchunks = (n + kScoreChunk - 1) / kScoreChunk;
  VG_HIP(b.partials.reserve_pow2((size_t)nchunks * kIekfVals + kIekfVals));
  PoseVar pose;
  for (int e = 0; e < 12; e++) pose.v[e] = pose12[e];
  for (int e = 12; e < 18; e++) pose.v[e] = 0.0;
  double* d_out = b.partials + (size_t)nchunks * kIekfVals;
  k_score_normal<<<nchunks, kScoreChunk, 0, s>>>(mp, ctx->map, b.xyz, n, pose, pose_var_arg(pose_var), b.partials);
  k_score_normal_sum<<<1, 64, 0, s>>>(b.partials, nchunks, d_out);
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(out34, d_out, kIekfVals * sizeof(double), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  return VG_OK;
}

}  // namespace vg

// Test / measurement hook: the device time of the last vg_score_poses call's
// kernels (HIP events on the context stream around them)
extern "C" int vgx_score_ms(vg_ctx* ctx, double* ms) {
  if (!ctx || !ms || !ctx->score.t.armed()) return VG_E_ARG;
  vg::KernelTimer& t = ctx->score.t;
  t.clear();
  VG_HIP(t.collect());
  *ms = t.ms;
  return VG_OK;
}
