// localizability.hip — the expected pose information of the map from a place
// (vg_localizability) and of a measured scan at a pose (vg_scan_info): the 6 x 6
// point-to-plane information matrix summed over rays, reduced on the device so
// that one 416-byte record per place (per scan) leaves it. The term, the
// reduction and the record's finish: vg_info.h.
//
// k_info_places: one 256-thread workgroup per place. Thread t casts directions
// t, t + 256, ... (ray_trace, as k_raycast: a latency-bound gather that lives on
// occupancy), so the lanes of a wave walk neighbouring directions of the table
// from one origin and meet the same headers in L1 / L2. After every 256
// directions each wave adds its lanes' terms in a shuffle tree and its first lane
// adds the result to the wave's 22 doubles of LDS: the sums do not live in
// registers across a walk (they would cost 44 VGPRs and a wave per SIMD). The
// workgroup's first lane adds the four waves' entries and finishes the record.
// Which lane meets which direction is a function of D alone, and nothing is shared between workgroups: a place's bytes do not
// depend on M, on its position or on the slab it falls in.
//
// k_info_scan: one lane per point through diff_point (vg_diff.h, the bits of
// vg_scan_diff), the CONSISTENT points' terms reduced per workgroup in the same
// tree into one InfoPart; k_info_scan_sum, one wave, lane k adding sum k over
// the workgroups in block order, then the same finish.
#include "vg_info.h"

namespace vg {

__global__ void __launch_bounds__(kInfoBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) k_info_places(double vs, DevMap m, const double* __restrict__ pos,
                                                               const double* __restrict__ dirs, int D, InfoPrm prm,
                                                               double dept2, double beam_dv,
                                                               vg_info_rec* __restrict__ out) {
  __shared__ InfoPart red[kInfoWaves];
  const int place = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const V3 o = ld_v3(pos + 3 * (size_t)place);
  if (lane == 0) {  // (the wave's entry: no other lane touches it before the workgroup's sum)
    for (int k = 0; k < kInfoSums; k++) red[wave].s[k] = 0.0;
    red[wave].n_hits = red[wave].flags = 0;
  }
  for (int i0 = 0; i0 < D; i0 += kInfoBlock) {  // (uniform trip count: every lane reaches the shuffles)
    const int i = i0 + threadIdx.x;
    double s[kInfoSums];
#pragma unroll
    for (int k = 0; k < kInfoSums; k++) s[k] = 0.0;
    int n_hits = 0, flags = 0;
    if (i < D) {
      const V3 dir = ld_v3(dirs + 3 * (size_t)i);
      vg_ray_hit h;
      ray_trace(m, vs, o, dir, prm.ray, h);
      flags = h.flags & kInfoEnded;
      if (h.flags & kRayHit) {
        const double dn = norm3(dir);  // (ray_trace's own normalisation)
        const V3 rd = v3(h.range * (dir[0] / dn), h.range * (dir[1] / dn), h.range * (dir[2] / dn));
        double J[6], w;
        if (info_term(rd, h.range, h, dept2, beam_dv, prm.floor_var, J, w)) {
          info_set(s, J, w);
          n_hits = 1;
        }
      }
    }
    info_wave_sum(s, n_hits, flags);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kInfoSums; k++) red[wave].s[k] += s[k];
      red[wave].n_hits += n_hits;
      red[wave].flags |= flags;
    }
  }
  __shared__ InfoPart tot;
  info_block_sum(red, tot);
  if (threadIdx.x == 0) info_finish(tot.s, D, tot.n_hits, tot.flags != 0, prm.min_hits, out[place]);
}

__global__ void __launch_bounds__(kInfoBlock) k_info_scan(MP mp, DevMap m, const float* __restrict__ xyz, int n,
                                                          Pose12 pose, DiffPrm prm, double floor_var,
                                                          InfoPart* __restrict__ part) {
  __shared__ InfoPart red[kInfoWaves];
  const int i = blockIdx.x * kInfoBlock + threadIdx.x;
  double s[kInfoSums];
#pragma unroll
  for (int k = 0; k < kInfoSums; k++) s[k] = 0.0;
  int n_hits = 0, flags = 0;
  if (i < n) {
    const V3 pb = v3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
    vg_diff_point dp;
    vg_ray_hit h;
    double av;
    int rflags;
    V3 w, o;
    diff_point(mp, m, pb, pose, prm, dp, av, rflags, w, o, h);
    flags = rflags & kInfoEnded;
    if (dp.cls == VG_DIFF_CONSISTENT) {
      double J[6], wt;
      if (info_term(sub(w, o), dp.r_meas, h, (double)mp.dept * (double)mp.dept, mp.beam_dv, floor_var, J, wt)) {
        info_set(s, J, wt);
        n_hits = 1;
      }
    }
  }
  info_wave_sum(s, n_hits, flags);
  if ((threadIdx.x & 63) == 0) {
    InfoPart& r = red[threadIdx.x >> 6];
#pragma unroll
    for (int k = 0; k < kInfoSums; k++) r.s[k] = s[k];
    r.n_hits = n_hits;
    r.flags = flags;
  }
  __shared__ InfoPart tot;
  info_block_sum(red, tot);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// one wave: lane k < 22 adds sum k over the workgroups in block order, lane 22 the hits, lane 23 ORs the flags
__global__ void __launch_bounds__(64) k_info_scan_sum(const InfoPart* __restrict__ part, int n_blocks, int n,
                                                      int min_hits, vg_info_rec* __restrict__ out) {
  __shared__ InfoPart tot;
  const int k = threadIdx.x;
  if (k < kInfoSums) {
    double s = 0.0;
    for (int b = 0; b < n_blocks; b++) s += part[b].s[k];
    tot.s[k] = s;
  } else if (k == kInfoSums) {
    int c = 0;
    for (int b = 0; b < n_blocks; b++) c += part[b].n_hits;
    tot.n_hits = c;
  } else if (k == kInfoSums + 1) {
    int f = 0;
    for (int b = 0; b < n_blocks; b++) f |= part[b].flags;
    tot.flags = f;
  }
  __syncthreads();
  if (k == 0) info_finish(tot.s, n, tot.n_hits, tot.flags != 0, min_hits, *out);
}

// ---- host side

static int info_bufs(vg_ctx* ctx) {
  InfoBufs& b = ctx->info;
  static_assert(sizeof(vg_info_rec) == 416 && sizeof(vg_info_params) == 112 && sizeof(InfoPart) == 184,
                "the records' documented sizes");
  const size_t slab = (size_t)(b.slab_want > 0 ? b.slab_want : kInfoSlab);
  const size_t pts = (size_t)(ctx->cap.max_points_per_scan > 0 ? ctx->cap.max_points_per_scan : 1);
  VG_HIP(b.pos.reserve(slab * 3));
  VG_HIP(b.dirs.reserve((size_t)kInfoMaxDirs * 3));
  VG_HIP(b.out.reserve(slab));
  VG_HIP(b.part.reserve((pts + kInfoBlock - 1) / kInfoBlock));
  return VG_OK;
}

int localizability_dev(vg_ctx* ctx, const MP& mp, const double* positions, int M, const double* dirs, int D,
                       const vg_info_params* prm, vg_info_rec* out) {
  if (M <= 0) return VG_OK;
  VG_TRY(info_bufs(ctx));
  InfoBufs& b = ctx->info;
  hipStream_t s = ctx->stream;
  const InfoPrm q = info_prm(prm);
  vg_info_rec* d_out = b.out;
  const int slab = (int)b.out.cap;
  b.t.clear();
  VG_HIP(hipMemcpyAsync(b.dirs, dirs, (size_t)D * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  for (int i0 = 0; i0 < M; i0 += slab) {
    const int m = M - i0 < slab ? M - i0 : slab;
    VG_HIP(hipMemcpyAsync(b.pos, positions + 3 * (size_t)i0, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    VG_HIP(b.t.begin(s));
    k_info_places<<<m, kInfoBlock, 0, s>>>(mp.vs, ctx->map, b.pos, b.dirs, D, q, (double)mp.dept * (double)mp.dept,
                                           mp.beam_dv, d_out);
    VG_HIP(b.t.end(s));
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(out + i0, d_out, (size_t)m * sizeof(vg_info_rec), hipMemcpyDeviceToHost, s));
    VG_HIP(hipStreamSynchronize(s));  // the slab's staging is reused by the next
    VG_HIP(b.t.collect());
  }
  return VG_OK;
}

int scan_info_dev(vg_ctx* ctx, const MP& mp, const float* xyz, int n, const double* pose12,
                  const vg_diff_params* diff, const vg_info_params* prm, vg_info_rec* out) {
  memset(out, 0, sizeof(*out));
  if (n <= 0) return VG_OK;
  VG_TRY(ray_bufs(ctx));
  VG_TRY(info_bufs(ctx));
  InfoBufs& b = ctx->info;
  hipStream_t s = ctx->stream;
  const DiffPrm dq = diff_prm(diff);
  const InfoPrm q = info_prm(prm);
  Pose12 pose;
  for (int e = 0; e < 12; e++) pose.v[e] = pose12[e];
  float* d_xyz = reinterpret_cast<float*>(ctx->ray.dir.p);  // (the cloud's staging of vg_scan_diff: n <= its capacity)
  InfoPart* d_part = b.part;
  vg_info_rec* d_out = b.out;
  const int n_blocks = (n + kInfoBlock - 1) / kInfoBlock;
  b.t.clear();
  VG_HIP(hipMemcpyAsync(d_xyz, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s));
  VG_HIP(b.t.begin(s));
  k_info_scan<<<n_blocks, kInfoBlock, 0, s>>>(mp, ctx->map, d_xyz, n, pose, dq, q.floor_var, d_part);
  k_info_scan_sum<<<1, 64, 0, s>>>(d_part, n_blocks, n, q.min_hits, d_out);
  VG_HIP(b.t.end(s));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(out, d_out, sizeof(vg_info_rec), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  VG_HIP(b.t.collect());
  return VG_OK;
}

}  // namespace vg

// Test / measurement hooks. vgx_info_ms: the device time of the last vg_localizability call's kernels, summed
// over its slabs, or of the last vg_scan_info call's (HIP events on the context stream around them).
// vgx_info_slab: the places per launch of vg_localizability from the next call on (<= 0: the default); the
// staging is freed and allocated again at that size
extern "C" int vgx_info_ms(vg_ctx* ctx, double* ms) {
  if (!ctx || !ms || !ctx->info.t.armed()) return VG_E_ARG;
  *ms = ctx->info.t.ms;
  return VG_OK;
}
extern "C" int vgx_info_slab(vg_ctx* ctx, int places) {
  if (!ctx) return VG_E_ARG;
  if (ctx->stream) VG_HIP(hipStreamSynchronize(ctx->stream));
  vg::InfoBufs& b = ctx->info;
  b.slab_want = places > 0 ? places : 0;
  b.pos.release();
  b.dirs.release();
  b.out.release();
  b.part.release();
  return VG_OK;
}
