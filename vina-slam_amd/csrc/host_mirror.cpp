// host_mirror.cpp — the host mirror of the device-resident estimator state
// (HostPipe, vg_host.h): its lifetime, its absorption of what the device
// publishes, and the accessors that read it.
//
// What is absorbed and when: each enqueued scan leaves a Pend with two
// publication numbers. P1 (the state block: x_curr, the window states, the
// trajectory row, the IEKF's counters) is published right after the BA; P2
// (the end-of-scan counters, which complete the scan's stats) after the margi.
// Nothing is absorbed when a scan is enqueued: the next host propagation or
// window push takes P1 of the newest scan (absorb), the insert takes every
// earlier scan whole, vg_poll takes what has arrived without waiting
// (absorb_ready), and host_sync drains the stream and takes everything.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "vg_host.h"

namespace vg {

void host_init(vg_ctx* ctx) {
  HostPipe* P = new HostPipe();
  const vg_config& c = ctx->cfg;
  P->mp.resize(c.win_size);
  for (int i = 0; i < c.win_size; i++) P->mp[i] = i;
  MP& m = P->mpd;
  memset(&m, 0, sizeof(m));
  m.vs = c.voxel_size;
  m.min_eig = c.min_eigen_value;
  for (int i = 0; i < 4; i++) {
    m.thre[i] = 1.0 / c.plane_eigen_value_thre[i];
    m.minpt[i] = c.min_point[i];
  }
  for (int i = 0; i < 9; i++) m.extR[i] = c.ext_R[i];
  for (int i = 0; i < 3; i++) m.extt[i] = c.ext_t[i];
  m.dept = (float)c.dept_err;
  m.beam = (float)c.beam_err;
  {
    const double sb = sin(m.beam * M_PI / 180.0);  // calcBodyVar's (float degree_inc) * M_PI / 180.0
    m.beam_dv = sb * sb;
  }
  m.max_layer = c.max_layer;
  m.max_points = c.max_points;
  m.W = c.win_size;
  for (int i = 0; i < 3; i++) {
    P->noiseMeas(i, i) = c.ba_cov_gyr;
    P->noiseMeas(3 + i, 3 + i) = c.ba_cov_acc;
    P->noiseWalk(i, i) = c.ba_rdw_gyr;
    P->noiseWalk(3 + i, 3 + i) = c.ba_rdw_acc;
  }
  P->sg = gravity_scale(c);
  if (c.cold_start) P->init = init_create(ctx);
  ctx->host = P;
}
void host_free(vg_ctx* ctx) {
  if (hp(ctx) && hp(ctx)->init) init_destroy(hp(ctx)->init);
  delete hp(ctx);
  ctx->host = nullptr;
}
void host_reset(vg_ctx* ctx) {
  host_free(ctx);
  host_init(ctx);
}

// ---- absorbing published device results into the host mirror

static int map_error(vg_ctx* ctx, int e) {
  ctx->err = std::string("device map error flags=") + std::to_string(e) + ((e & 4) ? " (node pool full)" : "") +
             ((e & 8) ? " (point_fix arena full)" : "") + ((e & 1) ? " (voxel key out of packed range)" : "") +
             ((e & 2) ? " (root hash full)" : "") + ((e & 16) ? " (subdivision event buffer full)" : "") +
             ((e & 32) ? " (sharded exchange out of step: the ranks' exchange sequences differ)" : "") +
             ((e & 64) ? " (cross-stream hand-off timed out)" : "");
  if (e & (32 | 64)) return VG_E_STATE;  // out-of-step exchange, or a hand-off that timed out: not a capacity limit
  return (e & 1) ? VG_E_RANGE : VG_E_CAPACITY;
}

// LioStateEstimation's return value (odometry.cpp:244-254): lambda_min of
// sum n n^T >= 14; bookkeeping only (degrade_cnt, local_mapping.cpp:413-423)
int degenerate_of(const double* nnt) {
  M3 nn;
  nn(0, 0) = nnt[0];
  nn(0, 1) = nn(1, 0) = nnt[1];
  nn(0, 2) = nn(2, 0) = nnt[2];
  nn(1, 1) = nnt[3];
  nn(1, 2) = nn(2, 1) = nnt[4];
  nn(2, 2) = nnt[5];
  V3 ev;
  M3 U;
  eig3(nn, ev, U);
  return (ev[0] < 14) ? 1 : 0;
}

// P1 of the oldest pending scan: x_curr, post-IEKF pose, window states
static int absorb_p1(vg_ctx* ctx, HostPipe* P, Pend& q) {
  if (q.seq1 == 0) return VG_OK;
  VG_TRY(pub_wait(ctx, &ctx->h_pub->seq1, q.seq1, "state publication"));
  const Pub& pb = *ctx->h_pub;
  HX& xc = P->x_curr;
  hx_get_block(xc, pb.xc);
  for (size_t i = 0; i < P->x_buf.size(); i++) hx_get_frame(P->x_buf[i], pb.xs + (i + q.shift) * kXS);
  if (q.pushed >= 0 && q.pushed < (int)P->x_buf.size()) P->x_buf[q.pushed].cov = xc.cov;
  if (!q.init_tail) {  // pub_localtraj's path point and save_pose_tum's row (local_mapping.cpp:427-430)
    P->traj.push_back(q.t);
    for (int i = 0; i < 12; i++) P->traj.push_back(pb.traj[i]);
    P->path.push_back(q.t);
    for (int i = 0; i < 12; i++) P->path.push_back(pb.traj[i]);
    P->path.push_back(P->jour);
    q.st.iekf_iters = pb.iekf_iters;
    for (int i = 0; i < 4; i++) q.st.iekf_matches[i] = pb.matches[i];
    q.st.iekf_points = pb.iekf_pts;
    q.st.degenerate = degenerate_of(pb.nnt);
  }
  q.st.ba_iters = pb.ba_iters1;
  q.st.ba_hess = pb.ba_hess1;
  for (int i = 0; i < 4; i++) q.st.iekf_planes[i] = pb.planes[i];
  if (q.shift) {  // pub_localmap (publishers.cpp:121-129, local_mapping.cpp:505): the window's path rows
                  // [win_base, win_base + win_count) take x_buf[i].p after the BA (pb.xs: the window before the slide)
    const int W = ctx->cfg.win_size;
    const int rows = (int)P->path.size() / kPathRow;
    if (rows >= W)
      for (int i = 0; i < W; i++) memcpy(&P->path[(size_t)(rows - W + i) * kPathRow + 10], pb.xs + (size_t)i * kXS + 9, 24);
  }
  if (q.jour_check) {  // local_mapping.cpp:525-533 with x_curr.p = x_buf.back().p after the BA
    double spat = norm3(sub(xc.p, P->last_pos));
    if (spat > 0.5) {
      P->jour += spat;
      P->last_pos = xc.p;
      P->release_flag = true;
    }
  }
  q.seq1 = 0;
  return VG_OK;
}

// k_iekf launches of the executed IEKF iterations (vg_profile bit 0)
static void collect_iekf_events(vg_ctx* ctx, const Pend& q) {
  for (int r = 0; r < q.ev_n && r < q.st.iekf_iters; r++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->iekf_ev[q.ev_base + r][0], ctx->iekf_ev[q.ev_base + r][1]) == hipSuccess) {
      ctx->prof_ms[kProfIekfKernel] += ms;
      ctx->prof_n[kProfIekfKernel] += 1;
    }
  }
}

// P2: end-of-scan counters; the scan's stats are complete
static int absorb_p2(vg_ctx* ctx, HostPipe* P, Pend& q) {
  VG_TRY(absorb_p1(ctx, P, q));
  VG_TRY(pub_wait(ctx, &ctx->h_pub->seq2, q.seq2, "counter publication"));
  const int* c = ctx->h_pub->counters;
  q.st.n_slide = c[kCntSlide];
  q.st.nodes_used = c[kCntNodes];
  q.st.fix_used = c[kCntFix];
  if (!q.init_tail) q.st.roots_new = c[kCntRoots];  // init: the rebuilt map's roots (init.cpp)
  q.st.plane_updates = c[kCntPlaneUpd];
  if (!q.init_tail) {  // the insert's downsampled count (the insert read it on the device)
    q.st.n_ds = c[kCntNds];
    if (q.ins_slot >= 0) P->wp_n[q.ins_slot] = c[kCntNds];
  }
  q.st.fix_full = c[kCntFixFull];
  q.st.v_ins = c[kCntSeg];
  if (q.frozen) {  // the counters are the last mapping scan's: nothing of this scan touched the map
    q.st.n_slide = q.st.roots_new = q.st.plane_updates = q.st.fix_full = q.st.v_ins = 0;
    q.st.n_ds = q.n_ds;  // the downsample's own count (no insert took it)
  }
  // events recorded while this scan was enqueued are complete now
  collect_iekf_events(ctx, q);
  for (int i = 0; i < kProfN; i++)
    if (ctx->prof_pending[i] && i != kProfIekfKernel) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ctx->prof_ev[i][0], ctx->prof_ev[i][1]) == hipSuccess) {
        ctx->prof_ms[i] += ms;
        ctx->prof_n[i] += 1;
      }
      ctx->prof_pending[i] = false;
    }
  ctx->stats = q.st;
  P->stats_log.push_back(q.st);
  if (c[kCntErr]) return map_error(ctx, c[kCntErr]);
  return VG_OK;
}

// The outcome of the previous fused step's LM (stage_ba left it pending):
// ba_resolve waits for its flags and enqueues any further iteration; if the
// speculative margi tail did not run, the real one follows with the same
// publication numbers and window view, so every wait already enqueued on
// those numbers (the next IEKF's hand-off flags, the host's P1 / P2) holds.
// block = false: returns without waiting when a flag is not published yet.
int resolve_lm(vg_ctx* ctx, HostPipe* P, bool block) {
  if (!P->lmp.active) return VG_OK;
  HostTimer ht_(ctx, kHostBA);
  bool fin = true, tail_ok = true;
  int iters = 0;
  int r = ba_resolve(ctx, block, &fin, &iters, &tail_ok);
  if (r == VG_OK && !fin) return VG_OK;
  P->lmp.active = false;
  if (r == VG_OK && !tail_ok)
    r = map_margi(ctx, P->mpd, P->lmp.wa, 0, ctx->cfg.thread_num, P->lmp.seq1, P->lmp.seq2, nullptr);
  if (r != VG_OK) P->sticky = r;
  return r;
}

// absorb every pending scan whose results are needed (all of P1, and P2 when
// `full`); blocking
int absorb(vg_ctx* ctx, HostPipe* P, bool full) {
  if (P->sticky != VG_OK) return P->sticky;
  VG_TRY(resolve_lm(ctx, P));
  int r = VG_OK;
  while (!P->pend.empty()) {
    Pend& q = P->pend.front();
    r = full || P->pend.size() > 1 ? absorb_p2(ctx, P, q) : absorb_p1(ctx, P, q);
    if (r != VG_OK) break;
    if (q.seq1 == 0 && (full || P->pend.size() > 1)) {
      P->pend.pop_front();
    } else {
      break;
    }
  }
  if (r != VG_OK) P->sticky = r;
  return r;
}

// non-blocking: absorb, oldest first, every pending scan whose publications
// (state and end-of-scan counters) have both arrived; stops at the first that
// has not. Only the newest pending scan can be unpublished (the host absorbs a
// scan's state before the next scan publishes), so the Pub block holds the
// scan being absorbed.
static int absorb_ready(vg_ctx* ctx, HostPipe* P) {
  if (P->sticky != VG_OK) return P->sticky;
  VG_TRY(resolve_lm(ctx, P, false));
  if (P->lmp.active) return VG_OK;  // the LM is still running: nothing of that scan is published
  while (!P->pend.empty()) {
    Pend& q = P->pend.front();
    if (q.seq1 != 0 && __atomic_load_n(&ctx->h_pub->seq1, __ATOMIC_ACQUIRE) < q.seq1) break;
    if (__atomic_load_n(&ctx->h_pub->seq2, __ATOMIC_ACQUIRE) < q.seq2) break;
    const int r = absorb_p2(ctx, P, q);
    if (r != VG_OK) {
      P->sticky = r;
      return r;
    }
    P->pend.pop_front();
  }
  return VG_OK;
}

int host_sync(vg_ctx* ctx) {
  HostPipe* P = hp(ctx);
  if (P->in_scan) {
    ctx->err = "host_sync inside a scan";
    return VG_E_STATE;
  }
  VG_TRY(resolve_lm(ctx, P));  // before the drain: it may enqueue work
  VG_HIP(stream_wait(ctx));
  return absorb(ctx, P, true);
}

// ---- accessors

void host_seed(vg_ctx* ctx, const double* s) { hx_get_state(hp(ctx)->x_curr, s); }

// x_curr now: between scans the absorbed host mirror; inside a scan (e.g.
// save_pose_tum right after VNC_lio, local_mapping.cpp:429) the device state
int host_state(vg_ctx* ctx, double* s) {
  HostPipe* P = hp(ctx);
  if (!P->in_scan) {
    VG_TRY(host_sync(ctx));
    hx_put_state(P->x_curr, s);
    return VG_OK;
  }
  VG_TRY(flush_deferred(ctx, P));
  double* h = ctx->h_stage;
  VG_HIP(hipMemcpyAsync(h, ctx->st->xc, kXC * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(stream_wait(ctx));
  s[0] = P->cur.t;
  memcpy(s + 1, h, kXC * sizeof(double));  // a state is t, then the device's block as it stands (vg_host.h)
  return VG_OK;
}
int host_window(vg_ctx* ctx, double* out) {
  HostPipe* P = hp(ctx);
  for (size_t i = 0; i < P->x_buf.size(); i++) hx_put_state(P->x_buf[i], out + kState * i);
  return (int)P->x_buf.size();
}
int host_win_count(vg_ctx* ctx) { return hp(ctx)->win_count; }
int host_traj(vg_ctx* ctx, double* out, int cap, int from) {
  HostPipe* P = hp(ctx);
  int n = (int)P->traj.size() / kTrajRow;
  const int k = from < n ? (n - from < cap ? n - from : cap) : 0;
  if (out && k > 0) memcpy(out, P->traj.data() + (size_t)from * kTrajRow, (size_t)k * kTrajRow * sizeof(double));
  return n;
}
int host_path(vg_ctx* ctx, double* out, int cap) {
  HostPipe* P = hp(ctx);
  int n = (int)P->path.size() / kPathRow;
  if (out) memcpy(out, P->path.data(), (size_t)(n < cap ? n : cap) * kPathRow * sizeof(double));
  return n;
}
int host_poll(vg_ctx* ctx) {
  HostPipe* P = hp(ctx);
  if (P->in_scan) return VG_OK;  // a stage-level scan is open: nothing to absorb mid-scan
  return absorb_ready(ctx, P);
}
int host_stats_log(vg_ctx* ctx, vg_stats* out, int cap) {
  HostPipe* P = hp(ctx);
  int n = (int)P->stats_log.size();
  if (out)
    for (int i = 0; i < n && i < cap; i++) out[i] = P->stats_log[i];
  return n;
}

}  // namespace vg
