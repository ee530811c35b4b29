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
#include "vg_ray.h"

namespace vg {

constexpr int kRayBlock = 256;

struct Pose12 {
  double v[12];
};

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

// sum: the summary's six counts (zeroed by the caller); absv: per point |range - r| where consistent, else 0
__global__ void __launch_bounds__(kRayBlock) k_scan_diff(MP mp, DevMap m, const float* __restrict__ xyz, int n,
                                                         Pose12 pose, RayPrm prm, double gate_sigma, double gate_floor,
                                                         vg_diff_point* __restrict__ pp, double* __restrict__ absv,
                                                         int* __restrict__ sum) {
  const int i = blockIdx.x * kRayBlock + threadIdx.x;
  const bool valid = i < n;
  int cls = -1, rflags = 0;
  if (valid) {
    const M3 R = ld_m3(pose.v);
    const V3 p = ld_v3(pose.v + 9);
    const V3 o = rigid(R, ld_v3(mp.extt), p);
    const V3 pb = v3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
    const V3 w = rigid(R, rigid(ld_m3(mp.extR), pb, ld_v3(mp.extt)), p);
    const V3 dv = sub(w, o);
    const double r = norm3(dv);
    const double dept2 = (double)mp.dept * (double)mp.dept, beam2 = r * r * mp.beam_dv;
    const double mc2 = prm.min_cos * prm.min_cos;
    RayPrm q = prm;
    const double reach = r + (gate_sigma * sqrt(dept2 + beam2 * (1.0 - mc2) / mc2) + 1.0);
    if (reach < q.t_max) q.t_max = reach;
    vg_ray_hit h;
    ray_trace(m, mp.vs, o, dv, q, h);
    rflags = h.flags;
    vg_diff_point dp;
    dp.cls = VG_DIFF_UNKNOWN;
    dp.leaf = -1;
    dp.r_meas = r;
    dp.r_map = 0.0;
    dp.gate = 0.0;
    double av = 0.0;
    if (h.flags & kRayHit) {
      const double c2 = h.ndotd * h.ndotd;
      double g2 = gate_sigma * gate_sigma * (h.var + dept2 + beam2 * (1.0 - c2) / c2);
      const double f2 = gate_floor * gate_floor;
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
    cls = dp.cls;
    if (pp) pp[i] = dp;
    absv[i] = av;
  }
  // the wave's counts: one atomic per class that occurs
  const int lane = threadIdx.x & 63;
  for (int c = 0; c < 6; c++) {
    const bool mine = c < 4 ? cls == c : (valid && (rflags & (c == 4 ? kRayTruncated : kRayOccupied)) != 0);
    const unsigned long long b = __ballot(mine);
    if (lane == 0 && b) atomicAdd(&sum[c], __popcll(b));
  }
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

static RayPrm ray_prm(const vg_ray_params* p) {
  RayPrm q;
  q.t_min = p ? p->t_min : 0.0;
  q.t_max = p && p->t_max > 0.0 ? p->t_max : 100.0;
  q.min_cos = p && p->min_cos > 0.0 ? p->min_cos : 0.05;
  q.max_steps = p && p->max_steps > 0 ? p->max_steps : 4096;
  q.pad = 0;
  return q;
}

static int ray_bufs(vg_ctx* ctx) {
  RayBufs& b = ctx->ray;
  if (b.cap > 0) return VG_OK;
  const size_t cap = (size_t)(ctx->cap.max_points_per_scan > 0 ? ctx->cap.max_points_per_scan : 1);
  static_assert(sizeof(vg_ray_hit) == 64 && sizeof(vg_diff_point) == 32, "the records' documented sizes");
  VG_HIP(hipMalloc(reinterpret_cast<void**>(&b.org), cap * 3 * sizeof(double)));
  VG_HIP(hipMalloc(reinterpret_cast<void**>(&b.dir), cap * 3 * sizeof(double)));
  VG_HIP(hipMalloc(&b.out, cap * sizeof(vg_ray_hit)));
  VG_HIP(hipMalloc(&b.sum, sizeof(vg_diff_summary)));
  for (auto& e : b.ev) VG_HIP(hipEventCreate(&e));
  b.cap = (int)cap;
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
  vg_ray_hit* d_out = static_cast<vg_ray_hit*>(b.out);
  if (shared) VG_HIP(hipMemcpyAsync(b.org, origins, 3 * sizeof(double), hipMemcpyHostToDevice, s));
  for (int i0 = 0; i0 < n; i0 += b.cap) {
    const int m = n - i0 < b.cap ? n - i0 : b.cap;
    if (!shared)
      VG_HIP(hipMemcpyAsync(b.org, origins + 3 * (size_t)i0, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    VG_HIP(hipMemcpyAsync(b.dir, dirs + 3 * (size_t)i0, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    VG_HIP(hipEventRecord(b.ev[0], s));
    k_raycast<<<(m + kRayBlock - 1) / kRayBlock, kRayBlock, 0, s>>>(mp.vs, ctx->map, b.org, shared, b.dir, m, q, d_out);
    VG_HIP(hipEventRecord(b.ev[1], s));
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
  const RayPrm q = ray_prm(prm ? &prm->ray : nullptr);
  const double gs = prm && prm->gate_sigma > 0.0 ? prm->gate_sigma : 3.0;
  const double gf = prm && prm->gate_floor > 0.0 ? prm->gate_floor : 0.0;
  Pose12 pose;
  for (int e = 0; e < 12; e++) pose.v[e] = pose12[e];
  float* d_xyz = reinterpret_cast<float*>(b.dir);
  vg_diff_point* d_pp = per_point ? static_cast<vg_diff_point*>(b.out) : nullptr;
  vg_diff_summary* d_sum = static_cast<vg_diff_summary*>(b.sum);
  VG_HIP(hipMemcpyAsync(d_xyz, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemsetAsync(d_sum, 0, sizeof(vg_diff_summary), s));
  VG_HIP(hipEventRecord(b.ev[0], s));
  k_scan_diff<<<(n + kRayBlock - 1) / kRayBlock, kRayBlock, 0, s>>>(mp, ctx->map, d_xyz, n, pose, q, gs, gf, d_pp, b.org,
                                                                   reinterpret_cast<int*>(d_sum));
  k_diff_sum<<<1, kRayBlock, 0, s>>>(b.org, n, d_sum);
  VG_HIP(hipEventRecord(b.ev[1], s));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(out, d_sum, sizeof(vg_diff_summary), hipMemcpyDeviceToHost, s));
  if (per_point) VG_HIP(hipMemcpyAsync(per_point, d_pp, (size_t)n * sizeof(vg_diff_point), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  return VG_OK;
}

void ray_free(vg_ctx* ctx) {
  RayBufs& b = ctx->ray;
  if (b.org) (void)hipFree(b.org);
  if (b.dir) (void)hipFree(b.dir);
  if (b.out) (void)hipFree(b.out);
  if (b.sum) (void)hipFree(b.sum);
  for (auto& e : b.ev)
    if (e) (void)hipEventDestroy(e);
  b = RayBufs();
}

}  // namespace vg

// Test / measurement hook: the device time of the last vg_raycast slab's or
// vg_scan_diff call's kernels (HIP events on the context stream around them)
extern "C" int vgx_ray_ms(vg_ctx* ctx, double* ms) {
  if (!ctx || !ms || !ctx->ray.ev[0]) return VG_E_ARG;
  float t = 0;
  VG_HIP(hipEventElapsedTime(&t, ctx->ray.ev[0], ctx->ray.ev[1]));
  *ms = t;
  return VG_OK;
}
