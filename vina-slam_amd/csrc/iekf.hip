// iekf.hip — the IEKF hot loop over the device-resident voxel map.
//
// SURVEY §8(a) rows:
//   A7  match / OctoTree::match / inside  voxel_map.cpp:241-266, octree.cpp:551-595, 732-737
//   A9  LioStateEstimation point loop     odometry.cpp:111-148
#include <hipcub/hipcub.hpp>
#include "vg_match.h"

namespace vg {

// ------------------------------------------------------------------ IEKF
// One IEKF iteration's point loop (odometry.cpp:111-148): world covariance,
// association (cached-leaf fast path or root hash + octree descent), the
// probabilistic point-to-plane gate (octree.cpp:557-579), the Jacobian and the
// weighted normal-equation accumulation. Each block writes 34 partial sums:
// HTH (upper 21), HTz (6), nnt (upper 6), match count (1). fp64 throughout.
// (descend, match_leaf, inside, the matched point's sums and the halving wave
// sums: vg_match.h, shared with score.hip)

// (iekf_points, the point loop of one workgroup, and pose_word / pose_of: vg_match.h,
// shared with the fleet's batched launches, fleet.hip)

template <bool kPf>
__global__ void __launch_bounds__(256) k_iekf(MP mp, DState* __restrict__ st, int it, DevMap m,
                                              int* __restrict__ cache, double* __restrict__ partials,
                                              int* __restrict__ pk) {
  if (st->done) return;
  // the scan's critical chain: its waves issue ahead of co-resident waves of
  // the previous scan's margi remainder (k_margi_copy) on a shared SIMD
  __builtin_amdgcn_s_setprio(2);
  const bool clk_on = st->clk.on != 0;
  const int clk_slot = (st->clk.scan * 4 + it) & (kClkRing - 1);
  if (clk_on && blockIdx.x == 0 && threadIdx.x == 0) {
    st->clk.t0[clk_slot] = (unsigned long long)wall_clock64();
    st->clk.exec[clk_slot] = 1;
  }
  VG_PROBE_BEGIN();
  double w[30];
  for (int t = 0; t < 30; t++) w[t] = pose_word(st->xc, t);
  M3 R, rot_var, tsl_var;
  V3 p;
  pose_of(w, R, p, rot_var, tsl_var);
  // XCD-aware chunking (cdna_hip_programming.md T1): blocks are dealt
  // round-robin over the 8 XCDs, so block b works on chunk (b % 8) * (nb / 8)
  // + b / 8 — each XCD sweeps a contiguous run of the scan and the plane /
  // node records of neighbouring points stay in its own L2 (nb % 8 == 0)
  const int nb = gridDim.x;
  const int vb = iekf_chunk(blockIdx.x, nb);
  double acc[kIekfVals];
  iekf_points<kPf>(mp, st, m, cache, pk, it, nb, vb, R, p, rot_var, tsl_var, acc);
  if (blockIdx.x == 0 && threadIdx.x == 0) st->iekf_pts += iekf_n(st);  // (vg_stats::iekf_points)
  if (blockIdx.x == 0) VG_PROBE_MARK(30);  // the point loop (thread 0 of block 0)
  __shared__ double red[4][kIekfVals];
  const double v = iekf_wg_sum(acc, red);
  if (threadIdx.x < kIekfVals) partials[(size_t)blockIdx.x * kIekfVals + threadIdx.x] = v;
  if (clk_on && blockIdx.x < kClkBlocks) {  // the workgroup's end (its partials written)
    __syncthreads();
    if (threadIdx.x == 0) st->clk.tend[clk_slot][blockIdx.x] = (unsigned long long)wall_clock64();
  }
  if (blockIdx.x == 0) VG_PROBE_MARK(31);  // the block reduction
#ifdef VG_PROBE
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g_probe[59], 1ull);
#endif
}

// the IEKF's end to the insert's stream (vg_ctx::d_sync[1]): every thread's
// state writes released at agent scope (one workgroup: one L2 write-back),
// then the flag advances by one
__device__ __forceinline__ void iekf_signal_done(unsigned* flag) {
  if (!flag) return;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(flag, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// P_k of SURVEY 8(d), the profiling pass only: distinct plane records the
// iteration read, deduplicated with a per-node tag (outside k_iekf's timing)
__global__ void __launch_bounds__(256) k_iekf_planes(const DState* __restrict__ st, DevMap m,
                                                     const int* __restrict__ pk, int tag, int* __restrict__ out) {
  if (st->done) return;
  const int* keep = iekf_keep(st);
  const int n = iekf_n(st);
  int cnt = 0;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    const int leaf = pk[keep ? keep[q] : q];
    if (leaf >= 0 && m.stamp[leaf] != tag && atomicExch(&m.stamp[leaf], tag) != tag) cnt++;
  }
  wave_append(out, cnt);
}

// The IEKF update of iteration `it` (vg_iekf.h) as its own one-workgroup
// launch. (A last-workgroup-done ticket inside k_iekf would need an
// agent-scope release per workgroup, which on the multi-XCD MI355X writes back
// the XCD's L2 each time: measured ~20 us per iteration, far more than the
// launch it saves.)
// done_flag: the update that finishes the IEKF also advances the IEKF ->
// insert hand-off flag (one workgroup: one release), so no k_sync_set launch
// follows the IEKF graph
__global__ void __launch_bounds__(1024) k_iekf_update(int nb, const double* __restrict__ partials,
                                                     DState* __restrict__ st, int it, unsigned* done_flag,
                                                     int xworld, int* xerr) {
  __shared__ IekfLds L;
  if (st->done) return;
  __builtin_amdgcn_s_setprio(2);  // (k_iekf)
  iekf_update_block(nb, partials, st, it, L, xworld, xerr);
  if (done_flag && L.fin) iekf_signal_done(done_flag);
}
// sharded mode: this shard's 34 sums (the update then runs on the all-reduced ones)
// sharded mode: this shard's 34 sums, packed into the exchange frame (the
// update runs on the all-reduced frame, k_iekf_update checks its guard); an
// iteration after convergence still closes the frame (the exchange runs)
__global__ void __launch_bounds__(1024) k_iekf_reduce(int nb, const double* __restrict__ partials,
                                                     const DState* __restrict__ st, XchgArg xa) {
  __shared__ IekfLds L;
  const bool done = st->done;
  if (!done) {
    const int n = iekf_n(st);
    iekf_reduce_block(nb, partials, L, n < nb * 256 ? (n + 255) / 256 : nb);
  }
  for (int i = threadIdx.x; i < xa.n - 2; i += blockDim.x) xa.frame[i] = (!done && i < kIekfVals) ? L.o[i] : 0.0;
  if (threadIdx.x == 0) xchg_close(xa.frame, xa.n, 0, xa.seq);
}

// grid of the IEKF point loop: sized by the context's capacity (the kernels
// read the scan size from the device state), a multiple of the 8 XCDs
static int iekf_blocks(vg_ctx* ctx) {
  return ((grid_for(ctx->cap.max_points_per_scan, 256, 512) + 7) / 8) * 8;
}
int iekf_grid(vg_ctx* ctx) { return iekf_blocks(ctx); }

// one IEKF iteration: the point loop (block partials) and the update; the
// optional event pair brackets k_iekf alone (vg_profile)
int iekf_iteration(vg_ctx* ctx, const MP& mp, const float* x, const float* y, const float* z, int n, int it,
                   hipEvent_t ev0, hipEvent_t ev1, int tag, hipStream_t s, unsigned* done_flag) {
  Work& w = ctx->wk;
  if (!s) s = ctx->stream;
  (void)x;
  (void)y;
  (void)z;
  (void)n;  // the scan is read from the device state (state_set_scan)
  const int nb = iekf_blocks(ctx);
  if (ev0) VG_HIP(hipEventRecord(ev0, s));
  auto kern = ctx->iekf_prefetch ? k_iekf<true> : k_iekf<false>;
  kern<<<nb, 256, 0, s>>>(mp, ctx->st, it, ctx->map, w.iekf_cache, w.partials, tag ? w.pk_leaf : nullptr);
  if (ev1) VG_HIP(hipEventRecord(ev1, s));
  if (tag) k_iekf_planes<<<nb, 256, 0, s>>>(ctx->st, ctx->map, w.pk_leaf, tag, &ctx->st->planes[it]);
  if (sharded(ctx)) {  // this shard's sums packed into the frame, all-reduced, then the (replicated) update
    Shard& sh = ctx->shard;
    const XchgArg xa{sh.d_frame, sh.d_seq, ctx->map.counters + kCntErr, kShardSmall, sh.world};
    k_iekf_reduce<<<1, 1024, 0, s>>>(nb, w.partials, ctx->st, xa);  // (the unsharded update's 60 row groups)
    VG_TRY(shard_exchange(ctx, kShardSmall, s));
    k_iekf_update<<<1, 1024, 0, s>>>(-1, sh.d_frame, ctx->st, it, nullptr, sh.world, ctx->map.counters + kCntErr);
  } else {
    k_iekf_update<<<1, 1024, 0, s>>>(nb, w.partials, ctx->st, it, done_flag, 0, nullptr);
  }
  VG_HIP(hipGetLastError());
  return VG_OK;
}

// ---- sharded mode (world > 1): the scan's points this rank can match ----
// A point is matched only in its own root voxel (A7, voxel_map.cpp:241-266),
// and only the owner of the voxel's tile holds it. At the
// scan's opening pose each raw point's world position w is taken with a box of
// kKeepM metres around it; the key rule is monotone in each coordinate, so
// the voxel keys of the box are those between the keys of w - kKeepM and
// w + kKeepM, and the point is kept when a tile of those keys is this rank's:
// one pass and a prefix sum per scan, and the IEKF's four iterations then
// transform and test only those (DState::skeep). The list holds while every
// point moved less than kmargin = kKeepM since the opening (iekf_keep, checked
// per iteration on the device), else the iteration takes every point. owns()
// still decides per point and iteration, so the matches are the unsharded
// path's either way; only the order of the fp sums within a rank follows the
// list.
constexpr double kKeepM = 0.1;
__global__ void __launch_bounds__(256) k_keep_flags(MP mp, const DState* __restrict__ st, DevMap m,
                                                    int* __restrict__ flag, unsigned* __restrict__ rmax_bits) {
  const int n = st->sn;
  const float* __restrict__ x = st->sx;
  const float* __restrict__ y = st->sy;
  const float* __restrict__ z = st->sz;
  M3 R;
  for (int q = 0; q < 9; q++) R[q] = st->xc[q];
  const V3 p = v3(st->xc[9], st->xc[10], st->xc[11]);
  const M3 eR = ld_m3(mp.extR);
  const V3 et = ld_v3(mp.extt);
  float rmax = 0.0f;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const V3 pnt = rigid(eR, v3(x[i], y[i], z[i]), et);
    const V3 w = rigid(R, pnt, p);
    rmax = fmaxf(rmax, (float)norm3(pnt));
    int64_t lo[3], hi[3];
    bool in = true;
    for (int j = 0; j < 3; j++) {
      const int64_t k0 = key_axis_d(w[j] - kKeepM, mp.vs) + kKeyOff, k1 = key_axis_d(w[j] + kKeepM, mp.vs) + kKeyOff;
      lo[j] = (k0 > 0 ? k0 : 0) >> 4;  // (keys outside the packed range are never matched)
      hi[j] = (k1 < 2 * kKeyOff - 1 ? k1 : 2 * kKeyOff - 1) >> 4;
      in &= k1 >= 0 && k0 < 2 * kKeyOff;
    }
    int keep = 0;
    if (in)
      for (int64_t tx = lo[0]; tx <= hi[0] && !keep; tx++)
        for (int64_t ty = lo[1]; ty <= hi[1] && !keep; ty++)
          for (int64_t tz = lo[2]; tz <= hi[2] && !keep; tz++)
            keep = tile_owner_t((uint64_t)tx, (uint64_t)ty, (uint64_t)tz, m.shard_world) == m.shard_rank;
    flag[i] = keep;
  }
  for (int off = 32; off > 0; off >>= 1) rmax = fmaxf(rmax, __shfl_down(rmax, off, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(rmax_bits, __float_as_uint(rmax));  // (non-negative: ordered as bits)
}
__global__ void __launch_bounds__(256) k_keep_scatter(MP mp, DState* __restrict__ st, const int* __restrict__ flag,
                                                      const int* __restrict__ pos, int* __restrict__ list,
                                                      const unsigned* __restrict__ rmax_bits) {
  const int n = st->sn;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    if (flag[i]) list[pos[i]] = i;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->snk = n > 0 ? pos[n - 1] + flag[n - 1] : 0;
    st->skeep = list;
    for (int t = 0; t < 12; t++) st->kpose[t] = st->xc[t];
    st->krmax = (double)__uint_as_float(*rmax_bits) * (1.0 + 1e-6) + 1e-6;  // (the float max rounded up)
    st->kmargin = kKeepM;
  }
}
static int keep_list(vg_ctx* ctx, const MP& mp, int n, hipStream_t s) {
  Shard& sh = ctx->shard;
  if (n <= 0) n = 1;  // (an empty scan: the kernels read the count from the state)
  VG_HIP(hipMemsetAsync(sh.keep_rmax, 0, sizeof(unsigned), s));
  const int g = grid_for(n);
  k_keep_flags<<<g, kBlock, 0, s>>>(mp, ctx->st, ctx->map, sh.keep_flag, sh.keep_rmax);
  size_t tb = sh.keep_tmp_bytes;
  VG_HIP(hipcub::DeviceScan::ExclusiveSum(sh.keep_tmp, tb, sh.keep_flag, sh.keep_pos, n, s));
  k_keep_scatter<<<g, kBlock, 0, s>>>(mp, ctx->st, sh.keep_flag, sh.keep_pos, sh.keep_list, sh.keep_rmax);
  VG_HIP(hipGetLastError());
  return VG_OK;
}

// the four IEKF iterations (odometry.cpp:68). The launches do not change from
// scan to scan, so an unsharded context captures them once and replays the
// graph: one host call instead of eight launches, and the device starts each
// node without the per-launch dispatch gap. The per-stage profiling pass
// (vg_profile bit 1) launches directly, with an event pair around each k_iekf.
int iekf_run(vg_ctx* ctx, const MP& mp, const float* x, const float* y, const float* z, int n, int bank,
             const double* begin_xc, hipStream_t s, const PropArg* begin_prop, bool signal, bool* signalled,
             bool opened) {
  if (!s) s = ctx->stream;
  if (signalled) *signalled = false;
  if (begin_xc || begin_prop)  // the scan opens here (pipeline.cpp)
    VG_TRY(state_scan_begin(ctx, begin_xc, x, y, z, n, s, begin_prop));
  else if (!opened) VG_TRY(state_set_scan(ctx, x, y, z, n, s));
  if (sharded(ctx) && ctx->shard.world > 1) VG_TRY(keep_list(ctx, mp, n, s));  // at the opening pose
  const bool graph = ctx->use_graphs && !sharded(ctx) && !ctx->prof_stages;
  const bool ev = ctx->prof_on && !graph;
  // the last update signals the hand-off itself (k_iekf_update; not when sharded)
  const bool self_signal = signal && !sharded(ctx);
  unsigned* flag = self_signal ? ctx->d_sync + 1 : nullptr;
  auto enqueue = [&]() -> int {
    for (int it = 0; it < 4; it++)
      VG_TRY(iekf_iteration(ctx, mp, x, y, z, n, it, ev ? ctx->iekf_ev[bank + it][0] : nullptr,
                            ev ? ctx->iekf_ev[bank + it][1] : nullptr,
                            graph || !ctx->prof_stages ? 0 : ++ctx->plane_tag, s, flag));
    return VG_OK;
  };
  if (!graph) {
    VG_TRY(enqueue());
    if (signalled) *signalled = self_signal;
    return VG_OK;
  }
  hipGraphExec_t& ge = ctx->g_iekf[self_signal ? 3 : 0];
  VG_TRY(capture_once(ctx, s, &ge, enqueue));
  VG_HIP(hipGraphLaunch(ge, s));
  if (signalled) *signalled = self_signal;
  return VG_OK;
}

// Test-only (vgx_memo_probe): the IEKF memo at centre planes. For every
// internal node, points exactly on its centre plane along each axis (the
// other two coordinates at +-hl/2) are looked up afresh (hash + descent, the
// reference's path: voxel_map.cpp:241-266, octree.cpp:586) and through the
// memo of the same point one ulp above / below the plane (the previous
// iteration's leaf). out: [0] samples, [1] memo != descent with the
// inclusive box (OctoTree::inside), [2] memo != descent with the descent's
// region (dbox, what k_iekf uses), [3] samples whose memo leaf differs from
// the fresh one (the plane really separates two leaves).
__global__ void __launch_bounds__(256) k_memo_probe(MP mp, DevMap m, int* __restrict__ out) {
  const int nn = m.counters[kCntNodes];
  int cnt[4] = {0, 0, 0, 0};
  for (int node = blockIdx.x * blockDim.x + threadIdx.x; node < nn; node += gridDim.x * blockDim.x) {
    const NodeHdr& h = m.hdr[node];
    if (h.octo != 1) continue;
    const double hl = h.qlen * 2;
    for (int j = 0; j < 3; j++)
      for (int sgn = 0; sgn < 4; sgn++)
        for (int side = 0; side < 2; side++) {
          V3 w = v3(h.center[0], h.center[1], h.center[2]);
          int k1 = (j + 1) % 3, k2 = (j + 2) % 3;
          w[k1] += ((sgn & 1) ? 0.5 : -0.5) * hl;
          w[k2] += ((sgn & 2) ? 0.5 : -0.5) * hl;
          V3 w2 = w;
          w2[j] = nextafter(w[j], side ? 1e300 : -1e300);
          uint64_t key, key2;
          if (!pack_key(w, mp.vs, key) || !pack_key(w2, mp.vs, key2) || key != key2) continue;
          const int root = hash_find(m.hkey, m.hval, m.hash_mask, key);
          if (root < 0) continue;
          const int fresh = descend(m.hdr, root, w), memo = descend(m.hdr, root, w2);
          if (fresh < 0 || memo < 0) continue;
          uint64_t kl;
          const NodeHdr& hm = m.hdr[memo];
          const bool same_root = pack_key(v3(hm.center[0], hm.center[1], hm.center[2]), mp.vs, kl) && kl == key;
          const int p_old = (same_root && inside(hm, w)) ? memo : fresh;
          const int p_new = (same_root && in_dbox(m.dbox + (size_t)memo * 6, w)) ? memo : fresh;
          cnt[0]++;
          cnt[1] += p_old != fresh;
          cnt[2] += p_new != fresh;
          cnt[3] += memo != fresh;
        }
  }
  for (int k = 0; k < 4; k++)
    if (cnt[k]) atomicAdd(&out[k], cnt[k]);
}
int map_memo_probe(vg_ctx* ctx, const MP& mp, int* out) {
  int* dout = reinterpret_cast<int*>(ctx->wk.partials);  // scratch: the probe runs between scans
  VG_HIP(hipMemsetAsync(dout, 0, 4 * sizeof(int), ctx->stream));
  k_memo_probe<<<256, 256, 0, ctx->stream>>>(mp, ctx->map, dout);
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(out, dout, 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(hipStreamSynchronize(ctx->stream));
  return VG_OK;
}

// Test-only (vgx_iekf_update): one k_iekf_update launch, as an IEKF iteration
// makes it, on given block partials (nb >= 0: nb x kIekfVals through the
// ordered reduction; nb < 0: the 34 final sums), states (250-double IMUST
// layout), iteration and rematch count. The device state's x_curr, x_prop, sn,
// rematch and done are overwritten, so use a context that is not stepped
// afterwards. x_out: x_curr after the update; G6_out (96 doubles): G(:, 0:6)
// 15 x 6 row-major, then the six nnt sums; flags_out: iters, matches[it],
// rematch, done.
int iekf_update_test(vg_ctx* ctx, int nb, const double* partials, int n_points, const double* x_curr,
                     const double* x_prop, int it, int rematch, double* x_out, double* G6_out, int* flags_out) {
  Work& w = ctx->wk;
  if (sharded(ctx) || it < 0 || it > 3 || nb == 0 || nb > w.nparts || n_points < 0 || rematch < 0) {
    ctx->err = "vgx_iekf_update: bad argument";
    return VG_E_ARG;
  }
  hipStream_t s = ctx->stream;
  DState* st = ctx->st;
  const size_t np = (nb < 0 ? 1 : (size_t)nb) * kIekfVals;
  const int zero = 0;
  VG_HIP(hipMemcpy(w.partials, partials, np * sizeof(double), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(st->xc, x_curr + 1, kXC * sizeof(double), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(st->xp, x_prop + 1, kXC * sizeof(double), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(&st->sn, &n_points, sizeof(int), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(&st->rematch, &rematch, sizeof(int), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(&st->done, &zero, sizeof(int), hipMemcpyHostToDevice));
  VG_HIP(hipDeviceSynchronize());  // (the context's stream does not wait for the null stream)
  k_iekf_update<<<1, 1024, 0, s>>>(nb, w.partials, st, it, nullptr, 0, nullptr);
  VG_HIP(hipGetLastError());
  VG_HIP(hipStreamSynchronize(s));
  int ints[9];  // it, rematch, done, iters, degenerate, matches[4]
  x_out[0] = x_curr[0];
  VG_HIP(hipMemcpy(x_out + 1, st->xc, kXC * sizeof(double), hipMemcpyDeviceToHost));
  VG_HIP(hipMemcpy(G6_out, st->G6, 90 * sizeof(double), hipMemcpyDeviceToHost));
  VG_HIP(hipMemcpy(G6_out + 90, st->nnt, 6 * sizeof(double), hipMemcpyDeviceToHost));
  VG_HIP(hipMemcpy(ints, &st->it, sizeof(ints), hipMemcpyDeviceToHost));
  flags_out[0] = ints[3];
  flags_out[1] = ints[5 + it];
  flags_out[2] = ints[1];
  flags_out[3] = ints[2];
  return VG_OK;
}

}  // namespace vg

#ifdef VG_PROBE
VG_PROBE_READER(vg_probe_read_iekf)
#endif
