// ckpt_host.cpp — the host mirror's part of a checkpoint (checkpoint.hip
// writes and reads the file): one byte blob, one section of the file.
// Saved: what the next scan reads of HostPipe (the pending queue is empty and
// no LM is outstanding after host_sync). Not saved: publication numbers and
// everything per-scan; stats_log restarts at the load.
#include <cstring>
#include <vector>

#include "ckpt_file.h"
#include "vg_host.h"

namespace vg {

int host_ckpt_allowed(vg_ctx* ctx, const char* who, bool save) {
  HostPipe* P = hp(ctx);
  const char* why = P->in_scan ? "a stage-level scan is open (vg_step_end first)"
                    : save && init_active(P) ? "the cold-start initialisation is still running (until init_phase 3)"
                    : ctx->shard.world > 1 ? "the context is sharded (world > 1)"
                                           : nullptr;
  if (!why) return save ? P->sticky : VG_OK;
  ctx->err = std::string(who) + ": " + why;
  return VG_E_STATE;
}

struct HostSnap {
  HX x_curr;
  std::vector<HX> x_buf;
  std::vector<std::vector<double>> recs;  // imu_pre: bg, ba, then the device record
  std::vector<int> mp;
  int win_count = 0, win_base = 0, epoch = 0, release_flag = 0, first = 0;
  double jour = 0, last_pcl_end_time = 0, sg = 1, last_pos[3] = {0, 0, 0};
  int wp_n[32] = {0};
  std::vector<double> traj, path;
  vg_stats stats;
};

void host_ckpt_blob(vg_ctx* ctx, std::vector<unsigned char>& out) {
  HostPipe* P = hp(ctx);
  BlobW w{out};
  double s[kState];
  hx_put_state(P->x_curr, s);
  w.f64s(s, kState);
  w.i64((int64_t)P->x_buf.size());
  for (const HX& x : P->x_buf) {
    hx_put_state(x, s);
    w.f64s(s, kState);
  }
  w.i64((int64_t)P->imu_pre.size());
  for (const HImuPre& q : P->imu_pre) {
    w.f64s(q.bg.a, 3);
    w.f64s(q.ba.a, 3);
    std::vector<double> rec(kBaImuRec, 0.0);
    if (q.rec.size() == (size_t)kBaImuRec) rec = q.rec;
    else q.record(rec.data());
    w.f64s(rec.data(), kBaImuRec);
  }
  w.i64((int64_t)P->mp.size());
  for (int v : P->mp) w.i64(v);
  w.i64(P->win_count);
  w.i64(P->win_base);
  w.i64(P->epoch);
  w.i64(P->release_flag ? 1 : 0);
  w.i64(P->first ? 1 : 0);
  w.f64(P->jour);
  w.f64(P->last_pcl_end_time);
  w.f64(P->sg);
  w.f64s(P->last_pos.a, 3);
  for (int i = 0; i < 32; i++) w.i64(P->wp_n[i]);
  w.i64((int64_t)P->traj.size());
  w.f64s(P->traj.data(), P->traj.size());
  w.i64((int64_t)P->path.size());
  w.f64s(P->path.data(), P->path.size());
  w.i64((int64_t)sizeof(vg_stats));
  w.raw(&ctx->stats, sizeof(vg_stats));
}

int host_ckpt_parse(vg_ctx* ctx, const unsigned char* p, size_t n, void** snap) {
  *snap = nullptr;
  HostSnap* S = new HostSnap();
  BlobR r{p, n};
  double s[kState];
  const int W = ctx->cfg.win_size;
  r.raw(s, sizeof(s));
  if (r.ok) hx_get_state(S->x_curr, s);
  const size_t nb = r.count(sizeof(s), 32);
  for (size_t i = 0; i < nb && r.ok; i++) {
    r.raw(s, sizeof(s));
    S->x_buf.emplace_back();
    hx_get_state(S->x_buf.back(), s);
  }
  const size_t ni = r.count((6 + kBaImuRec) * 8, 32);
  for (size_t i = 0; i < ni && r.ok; i++) {
    S->recs.emplace_back(6 + kBaImuRec);
    r.raw(S->recs.back().data(), (6 + kBaImuRec) * 8);
  }
  const size_t nm = r.count(8, 32);
  for (size_t i = 0; i < nm && r.ok; i++) S->mp.push_back((int)r.i64());
  S->win_count = (int)r.i64();
  S->win_base = (int)r.i64();
  S->epoch = (int)r.i64();
  S->release_flag = (int)r.i64();
  S->first = (int)r.i64();
  S->jour = r.f64();
  S->last_pcl_end_time = r.f64();
  S->sg = r.f64();
  r.raw(S->last_pos, 24);
  for (int i = 0; i < 32; i++) S->wp_n[i] = (int)r.i64();
  const size_t nt = r.count(8, (size_t)1 << 40);
  S->traj.resize(r.ok ? nt : 0);
  r.raw(S->traj.data(), nt * 8);
  const size_t np = r.count(8, (size_t)1 << 40);
  S->path.resize(r.ok ? np : 0);
  r.raw(S->path.data(), np * 8);
  const size_t ns = r.count(1, sizeof(vg_stats));
  memset(&S->stats, 0, sizeof(vg_stats));
  r.raw(&S->stats, ns);
  bool good = r.ok && r.at == n && ns == sizeof(vg_stats) && (int)nm == W && S->win_count >= 0 && S->win_count <= W &&
              (int)nb == S->win_count && ni == (nb > 0 ? nb - 1 : 0) && nt % kTrajRow == 0 && np % kPathRow == 0 &&
              S->win_base >= 0 && S->epoch >= 0;
  for (size_t i = 0; good && i < nm; i++) good = S->mp[i] >= 0 && S->mp[i] < W;
  for (int i = 0; good && i < 32; i++) good = S->wp_n[i] >= 0 && S->wp_n[i] <= ctx->cap.max_points_per_scan;
  if (!good) {
    delete S;
    return VG_E_ARG;
  }
  *snap = S;
  return VG_OK;
}

void host_ckpt_drop(void* snap) { delete (HostSnap*)snap; }

// after vg_reset: HostPipe is fresh (host_init)
void host_ckpt_install(vg_ctx* ctx, void* snap) {
  HostSnap* S = (HostSnap*)snap;
  HostPipe* P = hp(ctx);
  P->x_curr = S->x_curr;
  P->x_buf = S->x_buf;
  P->imu_pre.clear();
  for (const std::vector<double>& q : S->recs) {
    P->imu_pre.emplace_back(v3(q[0], q[1], q[2]), v3(q[3], q[4], q[5]));
    P->imu_pre.back().rec.assign(q.begin() + 6, q.end());
  }
  P->mp = S->mp;
  P->win_count = S->win_count;
  P->win_base = S->win_base;
  P->epoch = S->epoch;
  P->release_flag = S->release_flag != 0;
  P->first = S->first != 0;
  P->jour = S->jour;
  P->last_pcl_end_time = S->last_pcl_end_time;
  P->sg = S->sg;
  memcpy(P->last_pos.a, S->last_pos, 24);
  memcpy(P->wp_n, S->wp_n, sizeof(P->wp_n));
  P->traj.swap(S->traj);
  P->path.swap(S->path);
  ctx->stats = S->stats;
  if (P->init) init_finish(P->init);  // a saved context is past its cold start (host_ckpt_allowed)
  delete S;
}

}  // namespace vg
