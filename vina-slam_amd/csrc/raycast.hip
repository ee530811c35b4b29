// raycast.hip — rays through the voxel map to the first plane they meet
// (vg_raycast), and a scan checked against the ranges the map expects along
// its beams (vg_scan_diff). Both read the map only, through the traversal of
// vg_ray.h, so they run while mapping, in a frozen map, on an attached view
// and on a fleet's tracker alike.
//
// k_raycast / k_scan_diff: one lane per ray, 256-thread workgroups, no LDS.
// The kernel is a latency-bound gather: a ray's walk is a chain of dependent
// scattered loads (hash slot, 96 B headers down the octree, a 224 B plane
// record at a plane leaf) and the lanes of a wave diverge in its length, so
// the traversal keeps its state in registers (no stack, vg_ray.h) and the
// launch relies on occupancy to cover the latency. A ray's record has the same
// bits alone or anywhere in a batch: nothing is shared between lanes.
//
// vg_scan_diff's class counts are integer atomics, one per wave and class; the
// sum of |range - r| over the consistent points is stored per point and added
// by one workgroup in a fixed order (k_diff_sum), as k_score_sum does.
#include "vg_diff.h"

namespace vg {

__global__ void __launch_bounds__(kRayBlock) k_raycast(double vs, DevMap m, const double* __restrict__ org,
                                                       int shared_origin, const double* __restrict__ dir, int n,
                                                       RayPrm prm, vg_ray_hit* __restrict__ out) {
  const int i = blockIdx.x * kRayBlock + threadIdx.x;
  if (i >= n) return;
  const double* po = org + (shared_origin ? 0 : 3 * (size_t)i);
  const V3 o = ld_v3(po), d = ld_v3(dir + 3 * (size_t)i);
  vg_ray_hit r;
  ray_trace(m, vs, o, d, prm, r);
  out[i] = r;
}

// sum: the summary's six counts (zeroed by the caller); absv: per point |range - r| where consistent, else 0.
// The per-point body is vg_diff.h's, shared with k_change_accum (change.hip)
__global__ void __launch_bounds__(kRayBlock) k_scan_diff(MP mp, DevMap m, const float* __restrict__ xyz, int n,
                                                         Pose12 pose, DiffPrm prm, vg_diff_point* __restrict__ pp,
                                                         double* __restrict__ absv, int* __restrict__ sum) {
  const int i = blockIdx.x * kRayBlock + threadIdx.x;
  const bool valid = i < n;
  int cls = -1, rflags = 0;
  if (valid) {
    const V3 pb = v3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
    vg_diff_point dp;
    double av;
    V3 w;
    diff_point(mp, m, pb, pose, prm, dp, av, rflags, w);
    cls = dp.cls;
    if (pp) pp[i] = dp;
    absv[i] = av;
  }
  diff_wave_counts(cls, valid, rflags, sum);
}

// one workgroup: thread t adds the points t, t + 256, ... in that order, then a fixed tree over the threads
__global__ void __launch_bounds__(kRayBlock) k_diff_sum(const double* __restrict__ absv, int n,
                                                        vg_diff_summary* __restrict__ out) {
  __shared__ double red[kRayBlock];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n; i += kRayBlock) s += absv[i];
  red[t] = s;
  __syncthreads();
  for (int w = kRayBlock / 2; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) {
    out->sum_abs_consistent = red[0];
    out->reserved[0] = out->reserved[1] = out->reserved[2] = 0.0;
  }
}

// ---- host side

void diff_sum_launch(hipStream_t s, const double* absv, int n, vg_diff_summary* d_sum) {
  k_diff_sum<<<1, kRayBlock, 0, s>>>(absv, n, d_sum);
}

int ray_bufs(vg_ctx* ctx) {
  RayBufs& b = ctx->ray;
  const size_t cap = (size_t)(ctx->cap.max_points_per_scan > 0 ? ctx->cap.max_points_per_scan : 1);
  static_assert(sizeof(vg_ray_hit) == 64 && sizeof(vg_diff_point) == 32, "the records' documented sizes");
  VG_HIP(b.org.reserve(cap * 3));
  VG_HIP(b.dir.reserve(cap * 3));
  VG_HIP(b.out.reserve(cap));
  VG_HIP(b.sum.reserve(1));
  return VG_OK;
}

int raycast_dev(vg_ctx* ctx, const MP& mp, const double* origins, int n_origins, const double* dirs, int n,
                const vg_ray_params* prm, vg_ray_hit* out) {
  if (n <= 0) return VG_OK;
  VG_TRY(ray_bufs(ctx));
  RayBufs& b = ctx->ray;
  hipStream_t s = ctx->stream;
  const RayPrm q = ray_prm(prm);
  const int shared = n_origins == 1 && n > 1 ? 1 : 0;
  vg_ray_hit* d_out = b.out;
  const int cap = (int)b.out.cap;
  if (shared) VG_HIP(hipMemcpyAsync(b.org, origins, 3 * sizeof(double), hipMemcpyHostToDevice, s));
  for (int i0 = 0; i0 < n; i0 += cap) {
    const int m = n - i0 < cap ? n - i0 : cap;
    if (!shared)
      VG_HIP(hipMemcpyAsync(b.org, origins + 3 * (size_t)i0, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    VG_HIP(hipMemcpyAsync(b.dir, dirs + 3 * (size_t)i0, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    VG_HIP(b.t.begin(s));
    k_raycast<<<(m + kRayBlock - 1) / kRayBlock, kRayBlock, 0, s>>>(mp.vs, ctx->map, b.org, shared, b.dir, m, q, d_out);
    VG_HIP(b.t.end(s));
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(out + i0, d_out, (size_t)m * sizeof(vg_ray_hit), hipMemcpyDeviceToHost, s));
    VG_HIP(hipStreamSynchronize(s));  // the slab's staging is reused by the next
  }
  return VG_OK;
}

int scan_diff_dev(vg_ctx* ctx, const MP& mp, const float* xyz, int n, const double* pose12,
                  const vg_diff_params* prm, vg_diff_point* per_point, vg_diff_summary* out) {
  memset(out, 0, sizeof(*out));
  if (n <= 0) return VG_OK;
  VG_TRY(ray_bufs(ctx));
  RayBufs& b = ctx->ray;
  hipStream_t s = ctx->stream;
  const DiffPrm q = diff_prm(prm);
  Pose12 pose;
  for (int e = 0; e < 12; e++) pose.v[e] = pose12[e];
  float* d_xyz = reinterpret_cast<float*>(b.dir.p);
  vg_diff_point* d_pp = per_point ? reinterpret_cast<vg_diff_point*>(b.out.p) : nullptr;
  vg_diff_summary* d_sum = b.sum;
  VG_HIP(hipMemcpyAsync(d_xyz, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemsetAsync(d_sum, 0, sizeof(vg_diff_summary), s));
  VG_HIP(b.t.begin(s));
  k_scan_diff<<<(n + kRayBlock - 1) / kRayBlock, kRayBlock, 0, s>>>(mp, ctx->map, d_xyz, n, pose, q, d_pp, b.org,
                                                                   reinterpret_cast<int*>(d_sum));
  diff_sum_launch(s, b.org, n, d_sum);
  VG_HIP(b.t.end(s));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(out, d_sum, sizeof(vg_diff_summary), hipMemcpyDeviceToHost, s));
  if (per_point) VG_HIP(hipMemcpyAsync(per_point, d_pp, (size_t)n * sizeof(vg_diff_point), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  return VG_OK;
}

}  // namespace vg

// Test / measurement hook: the device time of the last vg_raycast slab's or
// vg_scan_diff call's kernels (HIP events on the context stream around them)
extern "C" int vgx_ray_ms(vg_ctx* ctx, double* ms) {
  if (!ctx || !ms || !ctx->ray.t.armed()) return VG_E_ARG;
  vg::KernelTimer& t = ctx->ray.t;
  t.clear();
  VG_HIP(t.collect());
  *ms = t.ms;
  return VG_OK;
}
