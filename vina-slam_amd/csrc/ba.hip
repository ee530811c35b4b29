// ba.hip — sliding-window LiDAR-inertial LM: the
// host driver. The kernels are in ba_factor.hip (factor passes, bookkeeping)
// and ba_solve.hip (the dense step); vg_ba.h holds what the three share, and
// vg_lm_loop.h the host loop's enqueue-ahead and stop rule.
//
// Replaces LI_BA_Optimizer::damping_iter (optimizers.cpp:430-517) with its
// divide_thread / only_residual / hess_plus (171-245, 340-376), the point-
// cluster factor LidarFactor::acc_evaluate2 / evaluate_only_residual
// (factors.cpp:22-158) and IMU_PRE::give_evaluate / update_state
// (imu_preintegration.cpp:97-163, 239-246).
//
// Per LM iteration, all device-resident, no host round trip:
//   k_ba_hess    one 512-lane workgroup per chunk of hess_fs(W) factors:
//                one lane per (factor, frame) evaluates Auk, the diagonal 6x6
//                block and the gradient piece (fp64 VALU); the off-diagonal
//                blocks, sums of rank-1 terms, are reduced as X^T S X on fp64
//                MFMA from LDS -> per-chunk partials (deterministic). The IMU
//                factors ride in the same launch (one workgroup each)
//   k_ba_hfinal  ordered sum of the chunk partials (sharded: into the exchange
//                frame, closed here)
//   k_ba_prep    assemble the 15W x 15W system (IMU blocks x imu_coef + LiDAR
//                6x6 blocks), gauge, Marquardt damping, pivoted tile image,
//                residual1 on the Hessian iterations
//   k_ba_solve   one 1024-lane workgroup: blocked LDL^T of the pivoted
//                system in LDS (16x16 tiles, MFMA f64 trailing updates), the trial
//                state and q1
//   k_ba_resid   a chunk of 256/W factors per workgroup step: merge clusters
//                at the trial poses, 3x3 eigen, write the trial eig/cluster
//                (the side effect margi consumes), chunk residual partials.
//                One more workgroup takes the IMU residuals at the trial state
//                and then, unsharded (vg_ctx::ba_fuse_ctl), the LM bookkeeping:
//                accept/reject, Nielsen damping update, bias restore,
//                convergence flag, the publication to the host
//   k_ba_rsum,   sharded only: the residual partials summed into the exchange
//   k_ba_control frame, and after the exchange the bookkeeping as a launch of
//                its own
// Launches folded into their neighbours where the context allows it:
//   k_ba_init_hess   the scan graph's first iteration (vg_ctx::ba_init_hess):
//                    k_ba_init + k_ba_hess as one launch
//   k_ba_resid_hess  the first iteration's residual pass (vg_ctx::ba_resid_hess):
//                    it also forms the second iteration's Hessian at the trial
//                    state, so that iteration has no k_ba_hess launch
// Kernels early-exit on the device-side `done` / `calc_hess` flags; the host
// enqueues one iteration ahead and reads `done` and the iteration count in
// between, as one published word (vg_lm_loop.h).
#include "vg_ba.h"

#include "vg_lm_loop.h"

namespace vg {

int ba_alloc(vg_ctx* ctx) {
  BaBufs& b = ctx->ba;
  const int W = ctx->cfg.win_size;
  b.cap_f = ctx->cap.max_nodes / 8 > 262144 ? 262144 : (ctx->cap.max_nodes / 8 > 4096 ? ctx->cap.max_nodes / 8 : 4096);
  const int L = 6 * W, nout = L * (L + 1) / 2 + L + 1, n = 15 * W;
  bool good = true;
  good &= (b.fac_node = ctx->arena.take<int>(b.cap_f)) != nullptr;
  good &= (b.fac_eig = ctx->arena.take<double>((size_t)b.cap_f * 12)) != nullptr;
  good &= (b.fac_pcr = ctx->arena.take<Clu>(b.cap_f)) != nullptr;
  good &= (b.hpart = ctx->arena.take<double>((size_t)(b.cap_f / hess_chunk(W) + 1) * nout)) != nullptr;
  good &= (b.hout = ctx->arena.take<double>(nout + 16)) != nullptr;
  good &= (b.hout_part = ctx->arena.take<double>(nout + 16)) != nullptr;
  good &= (b.rpart = ctx->arena.take<double>(kResidBlocks + 16)) != nullptr;
  // the staging area and the block carve() lays out, its two holes included
  // (vg_ba.h): the request is larger than the block and does not shrink
  good &= (b.xs = ctx->arena.take<double>(1024 + 2 * n * (n + 1) / 2 + 4 * n + kMaxNB * (kMaxNB + 1) / 2 * 256 + 4 * kMaxNB * kTile + 2 * kMaxW * kX + kMaxW * kImuRec +
                                          kMaxW * 12 + kMaxW * 931 + kMaxW + 64)) != nullptr;
  if (!good) {
    ctx->err = "arena exhausted (BA)";
    return VG_E_CAPACITY;
  }
  if (W > kMaxW || 15 * W > kMaxNB * kTile) {
    ctx->err = "win_size > 11 unsupported by the BA solve (LDS-resident 15W x 15W tile store)";
    return VG_E_ARG;
  }
  {  // both LM kernels keep their working set in LDS: check the device limit up front
    int lds_max = 0;
    VG_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    const size_t hess_total = hess_lds_bytes(W) + kHessThreads * sizeof(double);
    if (lds_max > 0 && (hess_total > (size_t)lds_max || solve_lds_bytes(W) > (size_t)lds_max)) {
      ctx->err = "LM kernels need " + std::to_string(hess_total) + " / " + std::to_string(solve_lds_bytes(W)) +
                 " B of LDS per workgroup; the device allows " + std::to_string(lds_max);
      return VG_E_ARG;
    }
  }
  VG_TRY(ba_solve_setup(ctx));
  return ba_factor_setup(ctx);
}

const int* ba_iters_dev(vg_ctx* ctx) { return &carve(ctx).st->iters; }
const int* ba_hess_dev(vg_ctx* ctx) { return &carve(ctx).st->nhess; }
const int* ba_gate_dev(vg_ctx* ctx) { return &carve(ctx).st->fin; }

// one LM iteration (optimizers.cpp:449-516); kernels early-exit on the
// device-side flags once converged. Every argument is fixed per context (the
// factor count, the flags and the publication number live on the device), so
// an unsharded run replays one captured graph per iteration; the sampled
// solve-timing runs launch directly (events around k_ba_solve).
// rh: 1 this iteration's residual pass is k_ba_resid_hess (it also forms the
// next iteration's Hessian at the trial), 2 this iteration's Hessian came
// from the previous iteration's k_ba_resid_hess (no k_ba_hess launch)
// ih (the scan graph, k == 0): k_ba_init_hess replaces k_ba_init + k_ba_hess
static void ba_iter_kernels(vg_ctx* ctx, int k, bool solve_ev, int& xerr, int rh = 0,
                            const InitHessArg* ih = nullptr) {
  const int W = ctx->cfg.win_size;
  hipStream_t s = ctx->stream;
  BaDev d = carve(ctx);
  const int nimu = W - 1;
  const int L = 6 * W, nl = L * (L + 1) / 2, nout = nl + L + 1;
  const bool shard_on = sharded(ctx);
  // (the factor count is read on the device, the recut's kCntFactors: fixed
  // grids, so an asynchronous recut needs no host round trip before the LM)
  const int nrb = kResidBlocks;
  Shard& sh = ctx->shard;
  // sharded: the Hessian / gradient / residual frame and the trial residual's
  // frame are packed by k_ba_hfinal / k_ba_rsum and checked by k_ba_prep /
  // k_ba_control (no pack / unpack launches)
  const double* hlx = shard_on ? sh.d_frame : d.hl;  // the LiDAR system the assembly reads
  CtlArg ctl{W, nimu, shard_on ? 1 : nrb, nl + L, ctx->cfg.imu_coef, hlx, d.imuout, d.imures,
             shard_on ? sh.d_frame : d.rpart, d.xs, d.xt, d.bias, d.st, ctx->d_pub, nullptr,
             shard_on ? sh.world : 0, ctx->map.counters + kCntErr};
  CtlArg ctl_fused = ctl;  // unsharded: the bookkeeping rides in k_ba_resid's IMU workgroup
  if (!shard_on && ctx->ba_fuse_ctl) ctl_fused.err = ctx->map.counters + kCntErr;
  if (ih) launch_ba_init_hess(ctx, d, *ih);
  else if (rh != 2) launch_ba_hess(ctx, d);
  const XchgArg xh{shard_on ? sh.d_frame : nullptr, sh.d_seq, ctx->map.counters + kCntErr, sh.frame_n, sh.world};
  launch_ba_hfinal(ctx, d, shard_on ? sh.d_frame : d.hl, xh);
  // sharded: every shard's factors -> one LiDAR Hessian / gradient / residual
  if (shard_on && xerr == VG_OK) xerr = shard_exchange(ctx, sh.frame_n);
  if (k == 0 && ctx->dbg_capture == 1 && ctx->dbg_cap_buf) {  // test knob (vgx_debug 5): the first pass
    (void)hipMemcpyAsync(ctx->dbg_cap_buf, d.hl, nout * sizeof(double), hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync(ctx->dbg_cap_buf + nout, d.imuout, (size_t)nimu * 931 * sizeof(double),
                         hipMemcpyDeviceToDevice, s);
    ctx->dbg_cap_n = nout + nimu * 931;
    ctx->dbg_capture = 2;
  }
  launch_prep_solve(ctx, d, hlx, shard_on ? sh.world : 0, solve_ev ? ctx->solve_ev[k] : nullptr);
  if (rh == 1) launch_ba_resid_hess(ctx, d, ctl_fused);
  else launch_ba_resid(ctx, d, ctl_fused);
  if (shard_on) {  // the residual over every shard's factors
    launch_ba_rsum(ctx, d, XchgArg{sh.d_frame, sh.d_seq, ctx->map.counters + kCntErr, kShardSmall, sh.world});
    if (xerr == VG_OK) xerr = shard_exchange(ctx, kShardSmall);
  }
  if (!ctl_fused.err) launch_ba_control(ctx, ctl);
}

static MpRing ba_ring(vg_ctx* ctx, const int* mp_ring) {
  MpRing ring;
  for (int i = 0; i < kMaxW; i++) ring.mp[i] = i < ctx->cfg.win_size ? mp_ring[i] : 0;
  return ring;
}
// the asynchronous recut left tras_opt's bookkeeping to the LM's first launch
static bool ba_take_finish(vg_ctx* ctx) {
  const bool fin = ctx->rc_finish_in_init;
  ctx->rc_finish_in_init = false;
  return fin;
}

// k_ba_init: seq0 > 0 the LM's first flag number, else (the scan graph) read
// on the device from DState::ph
// (the IMU records are in DState's ring (k_push_state), the mp ring rides in k_ba_init's arguments)
static void ba_init_kernel(vg_ctx* ctx, const int* mp_ring, int seq0) {
  launch_ba_init(ctx, carve(ctx), ba_ring(ctx, mp_ring), seq0, ba_take_finish(ctx));
}

// the two-iteration LM graphs take k_ba_resid_hess (unsharded, bookkeeping
// fused, hess_fs(W) two residual chunks)
static bool ba_rh_on(vg_ctx* ctx) {
  return ctx->ba_resid_hess && ctx->ba_fuse_ctl && !sharded(ctx) && resid_hess_ok(ctx->cfg.win_size);
}

// the scan graph's LM part (pipeline.cpp stage_insert_recut), captured on the
// context stream: k_ba_init reading its per-scan numbers from the device,
// then the first two iterations
int ba_capture_scan_lm(vg_ctx* ctx, const int* mp_ring) {
  int xerr = VG_OK;
  const bool rh = ba_rh_on(ctx);
  if (ctx->ba_init_hess && !sharded(ctx)) {  // k_ba_init inside the first Hessian pass
    const InitHessArg ih{ba_ring(ctx, mp_ring), ba_take_finish(ctx) ? 1 : 0, 0};
    ba_iter_kernels(ctx, 0, false, xerr, rh ? 1 : 0, &ih);
  } else {
    ba_init_kernel(ctx, mp_ring, 0);
    ba_iter_kernels(ctx, 0, false, xerr, rh ? 1 : 0);
  }
  ba_iter_kernels(ctx, 1, false, xerr, rh ? 2 : 0);
  VG_HIP(hipGetLastError());
  return xerr;
}

// Run damping_iter on the device state. The window states, the IMU records
// and the IMU bias records are read and written in DState.
// pre > 0: k_ba_init, the first `pre` iterations and the gated margi tail are
// already on the stream (the scan graph), with the flag numbers from
// ctx->ba_seq0_pre
// (win_size <= 11: ba_alloc fails context creation otherwise)
int ba_run(vg_ctx* ctx, int nf, const int* mp_ring, int* iters, const std::function<int()>& before_first_wait,
           const std::function<int(bool*)>& spec_tail, bool* tail_ok, bool* pending, int pre) {
  if (pending) *pending = false;
  const int W = ctx->cfg.win_size;
  hipStream_t s = ctx->stream;
  const bool shard_on = sharded(ctx);
  int seq0;
  // sharded (direct launches, exchanges between): k_ba_init inside the first
  // Hessian pass and the first residual pass forming the second iteration's
  // Hessian, as the unsharded graphs do; the residual's bookkeeping stays in
  // k_ba_control, behind the residual exchange
  const bool shard_fused = shard_on && ctx->ba_init_hess && ctx->ba_resid_hess && resid_hess_ok(W);
  InitHessArg ih;
  if (pre > 0) {
    seq0 = ctx->ba_seq0_pre;
  } else {
    seq0 = ctx->pub_seq + 1;
    ctx->pub_seq += 10;
    if (shard_fused) ih = InitHessArg{ba_ring(ctx, mp_ring), ba_take_finish(ctx) ? 1 : 0, seq0};
    else ba_init_kernel(ctx, mp_ring, seq0);
    VG_HIP(flush_insert_events(ctx));
  }
  int xerr = VG_OK;  // exchange errors (sharded mode)
  // k_ba_solve launch events (vg_profile): on every prof_every-th run only, so
  // that timing a long run costs the stream little (each record is a gap)
  const bool solve_ev = pre == 0 && ctx->prof_on && !ctx->prof_clock &&
                        (ctx->prof_every <= 1 || ctx->prof_runs++ % ctx->prof_every == 0);
  auto enqueue = [&](int k) {
    if (shard_fused && pre == 0 && k < 2) ba_iter_kernels(ctx, k, solve_ev, xerr, k + 1, k == 0 ? &ih : nullptr);
    else ba_iter_kernels(ctx, k, solve_ev, xerr);
  };
  const bool graph = ctx->use_graphs && ctx->ba_graph && !shard_on && !solve_ev && ctx->dbg_capture != 1;
  if (graph)
    VG_TRY(capture_once(ctx, s, &ctx->g_ba, [&]() {
      enqueue(0);
      return VG_OK;
    }));
  // the two iterations of the steady state as ONE graph (no graph boundary
  // between them: each boundary left the stream idle ~9 us)
  const bool graph2 = pre == 0 && graph && ctx->ba_graph2 && ctx->ba_last_iters >= 2;
  if (graph2)
    VG_TRY(capture_once(ctx, s, &ctx->g_ba2, [&]() {
      const bool rh = ba_rh_on(ctx);
      ba_iter_kernels(ctx, 0, solve_ev, xerr, rh ? 1 : 0);
      ba_iter_kernels(ctx, 1, solve_ev, xerr, rh ? 2 : 0);
      return VG_OK;
    }));
  BaLoop L;
  lm_loop_begin(L, seq0, pre);
  // iteration L.enq; an error reaches the caller at the loop's next check of xerr
  auto iteration = [&]() {
    if (!graph) {
      enqueue(L.enq);
      return VG_OK;
    }
    const hipError_t e = hipGraphLaunch(ctx->g_ba, s);
    if (e != hipSuccess && xerr == VG_OK) {
      ctx->err = std::string("hipGraphLaunch (LM iteration): ") + hipGetErrorString(e);
      xerr = VG_E_HIP;
    }
    return VG_OK;
  };
  if (graph2) {
    const hipError_t e = hipGraphLaunch(ctx->g_ba2, s);
    if (e != hipSuccess) {
      ctx->err = std::string("hipGraphLaunch (LM iterations 0-1): ") + hipGetErrorString(e);
      return VG_E_HIP;
    }
    L.enq = 2;
  } else if (pre == 0) {
    iteration();
    L.enq = 1;
  }
  const int r = lm_loop_advance(
      L, ctx->ba_last_iters, iteration,
      [&](int k) -> int {
        VG_HIP(hipGetLastError());
        VG_TRY(xerr);
        if (k == 0 && before_first_wait) VG_TRY(before_first_wait());
        if (spec_tail && lm_tail_due(L, ctx->ba_last_iters)) {
          bool queued = false;
          VG_TRY(spec_tail(&queued));
          if (queued) L.tail_at = L.enq;
        }
        // the outcome is read later (ba_resolve): the tail is queued, every
        // further iteration is a replay of the same graph
        return pending && L.tail_at > 0 && graph && !ctx->ba_no_defer ? kLmPause : VG_OK;
      },
      [&](int k, int* bw) -> int {
        VG_TRY(pub_wait(ctx, &ctx->h_pub->seq_ba, seq0 + k, "k_ba_control"));
        *bw = __atomic_load_n(&ctx->h_pub->ba_word, __ATOMIC_ACQUIRE);
        return VG_OK;
      });
  if (r == kLmPause) {
    L.active = true;
    ctx->ba_loop = L;
    *pending = true;
    *iters = -1;
    if (tail_ok) *tail_ok = true;
    return VG_OK;
  }
  if (r != kLmEnd) return r;
  const LmOutcome o = lm_loop_end(L);
  if (tail_ok) *tail_ok = o.tail_ok;
  *iters = o.iters;
  ctx->ba_last_iters = o.last_iters;
  if (solve_ev)  // k_ba_solve of the executed iterations only (the bench's roofline)
    for (int it = 0; it < o.iters && it < 10; it++) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ctx->solve_ev[it][0], ctx->solve_ev[it][1]) == hipSuccess) {
        ctx->prof_ms[kProfBaSolve] += ms;
        ctx->prof_n[kProfBaSolve] += 1;
      }
    }
  return VG_OK;
}

// The rest of a run that ba_run left pending, through the same loop
// (lm_loop_advance), every iteration a replay of the one-iteration graph.
int ba_resolve(vg_ctx* ctx, bool block, bool* finished, int* iters, bool* tail_ok) {
  BaLoop& L = ctx->ba_loop;
  *finished = true;
  if (!L.active) return VG_OK;
  const int r = lm_loop_advance(
      L, ctx->ba_last_iters,
      [&]() -> int {
        const hipError_t e = hipGraphLaunch(ctx->g_ba, ctx->stream);
        if (e == hipSuccess) return VG_OK;
        ctx->err = std::string("hipGraphLaunch (LM iteration): ") + hipGetErrorString(e);
        return VG_E_HIP;
      },
      [](int) { return VG_OK; },
      [&](int k, int* bw) -> int {
        if (!block && __atomic_load_n(&ctx->h_pub->seq_ba, __ATOMIC_ACQUIRE) < L.seq0 + k) return kLmNotYet;
        VG_TRY(pub_wait(ctx, &ctx->h_pub->seq_ba, L.seq0 + k, "k_ba_control"));
        *bw = __atomic_load_n(&ctx->h_pub->ba_word, __ATOMIC_ACQUIRE);
        return VG_OK;
      });
  if (r == kLmNotYet) {
    *finished = false;
    return VG_OK;
  }
  L.active = false;
  if (r != kLmEnd) return r;
  const LmOutcome o = lm_loop_end(L);
  *tail_ok = o.tail_ok;
  *iters = o.iters;
  ctx->ba_last_iters = o.last_iters;
  return VG_OK;
}

}  // namespace vg
