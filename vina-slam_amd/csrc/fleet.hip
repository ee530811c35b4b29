// fleet.hip — one frozen scan of B trackers in ten launches (vg_fleet_step_dev,
// fleet_host.cpp): the scan opening, the four IEKF iterations (point loop + update)
// and the publication, each launch covering every tracker of the fleet.
//
// The trackers are views of one owner's map (vg_map_attach), so one DevMap and
// one MP in the kernel arguments serve all; what differs per tracker comes from
// two tables indexed by the workgroup's tracker b: FleetIn (host-mapped, this
// step's opening, written by the host before the launches) and FleetTab (device,
// the tracker's DState, leaf cache, block partials and publication block).
//
// Every kernel writes only its tracker's memory: no device flag is polled, no
// ticket crosses workgroups and no word is shared between trackers. The device
// bodies are the lone path's (iekf_points, iekf_wg_sum, iekf_update_block,
// publish_state_block) on the same grid per tracker, so a tracker's sums, and
// with them its state, are a lone frozen context's bit for bit. The in-kernel
// clocks and the profiling pass (vg_profile) are not carried here.
//
// Grid of the point loop: dim3(nb, B), nb = the lone k_iekf grid (a multiple of
// 8). Workgroups are dealt to the 8 XCDs round-robin by their linear id
// blockIdx.x + nb * blockIdx.y, so with nb % 8 == 0 workgroup (x, b) lands on XCD
// x % 8 for every b: tracker b's chunks keep the lone kernel's XCD layout
// (iekf_chunk(blockIdx.x, nb), cdna_hip_programming.md T1), and the trackers
// that look at the same part of the shared map share its lines in that XCD's L2.
#include "vg_match.h"

namespace vg {

// k_scan_begin's work per tracker: x_curr after the propagation, x_prop, the
// IEKF flags and the scan binding; the step's active flag moves to the device
// (the other launches' workgroups read it there, not over the host link)
__global__ void __launch_bounds__(256) k_fleet_open(const FleetIn* __restrict__ in, const FleetTab* __restrict__ tab) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const FleetIn& a = in[b];
  const int active = a.active;
  if (tid == 0) *tab[b].act = active;
  if (!active) return;
  DState* __restrict__ st = tab[b].st;
  if (tid == 64) {
    st->sx = a.x;
    st->sy = a.y;
    st->sz = a.z;
    st->sn = a.n;
  }
  for (int t = tid; t < kXC; t += blockDim.x) {
    const double v = a.xc[t];
    st->xc[t] = v;
    st->xp[t] = v;
  }
  if (tid == 0) {
    st->it = 0;
    st->rematch = 0;
    st->done = 0;
    st->iters = 0;
    st->degenerate = 0;
    st->ticket = 0;
    for (int k = 0; k < 4; k++) st->matches[k] = 0;
    for (int k = 0; k < 4; k++) st->planes[k] = 0;
    st->iekf_pts = 0;
  }
}

// k_iekf's point loop for tracker blockIdx.y; at once out for a tracker that
// sits the step out or whose IEKF has finished
template <bool kPf>
__global__ void __launch_bounds__(256) k_fleet_iekf(MP mp, DevMap m, const FleetTab* __restrict__ tab, int it) {
  const FleetTab& T = tab[blockIdx.y];
  if (!*T.act) return;
  DState* __restrict__ st = T.st;
  if (st->done) return;
  __builtin_amdgcn_s_setprio(2);
  double w[30];
  for (int t = 0; t < 30; t++) w[t] = pose_word(st->xc, t);
  M3 R, rot_var, tsl_var;
  V3 p;
  pose_of(w, R, p, rot_var, tsl_var);
  const int nb = gridDim.x;
  const int vb = iekf_chunk(blockIdx.x, nb);
  double acc[kIekfVals];
  iekf_points<kPf>(mp, st, m, T.cache, nullptr, it, nb, vb, R, p, rot_var, tsl_var, acc);
  if (blockIdx.x == 0 && threadIdx.x == 0) st->iekf_pts += iekf_n(st);  // (vg_stats::iekf_points)
  __shared__ double red[4][kIekfVals];
  const double v = iekf_wg_sum(acc, red);
  if (threadIdx.x < kIekfVals) T.partials[(size_t)blockIdx.x * kIekfVals + threadIdx.x] = v;
}

// k_iekf_update for tracker blockIdx.x
__global__ void __launch_bounds__(1024) k_fleet_update(int nb, const FleetTab* __restrict__ tab, int it) {
  __shared__ IekfLds L;
  const FleetTab& T = tab[blockIdx.x];
  if (!*T.act) return;
  DState* __restrict__ st = T.st;
  if (st->done) return;
  __builtin_amdgcn_s_setprio(2);
  iekf_update_block(nb, T.partials, st, it, L);
}

// k_publish_state, then k_publish_counters, into the tracker's own Pub
__global__ void __launch_bounds__(256) k_fleet_publish(const FleetIn* __restrict__ in, const FleetTab* __restrict__ tab,
                                                      const int* __restrict__ counters) {
  const int b = blockIdx.x;
  const FleetTab& T = tab[b];
  if (!*T.act) return;
  const int win_count = in[b].win_count, seq1 = in[b].seq1, seq2 = in[b].seq2;
  publish_state_block(T.st, win_count, 0, nullptr, nullptr, T.pub, seq1);
  __syncthreads();
  const int t = threadIdx.x;
  if (t < kCntN) pub_store(&T.pub->counters[t], counters[t]);
  pub_drain();
  __syncthreads();
  if (t == 0) pub_flag(&T.pub->seq2, seq2);
}

int fleet_launch(hipStream_t s, const MP& mp, const DevMap& m, const FleetIn* in, const FleetTab* tab, int B, int nb,
                 bool prefetch, std::string* err) {
  k_fleet_open<<<B, 256, 0, s>>>(in, tab);
  auto kern = prefetch ? k_fleet_iekf<true> : k_fleet_iekf<false>;
  for (int it = 0; it < 4; it++) {
    kern<<<dim3(nb, B), 256, 0, s>>>(mp, m, tab, it);
    k_fleet_update<<<B, 1024, 0, s>>>(nb, tab, it);
  }
  k_fleet_publish<<<B, 256, 0, s>>>(in, tab, m.counters);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    *err = std::string("vg_fleet_step_dev: ") + hipGetErrorString(e);
    return VG_E_HIP;
  }
  return VG_OK;
}

}  // namespace vg
