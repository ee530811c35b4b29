// recut.hip — the recut of the device-resident voxel map (map.hip) and the
// factor extraction.
//
// SURVEY §8(a) rows:
//   A5  multi_recut -> OctoTree::recut    local_mapping.cpp:144-201, octree.cpp:257-393
//   A6  tras_opt (factor extraction)      octree.cpp:498-521
#include <cstdio>
#include "vg_map.h"

namespace vg {

// ------------------------------------------------------------------ recut (A5/A6)
// Level-synchronous OctoTree::recut (octree.cpp:335-393) with every count kept
// on the device: per level, k_rc_visit (worklist -> children / subdividing
// leaves / factor candidates), k_rc_win (window points of subdividing leaves)
// and k_rc_apply (one workgroup: deterministic child allocation, event sort in
// LDS, pushes in the reference's order). The host enqueues max_layer+1 levels
// and synchronizes once. A level whose subdivision exceeds the LDS capacity of
// k_rc_apply sets rc[kRcAbort]; the host then replays the rest of the recut
// with the host-sized path (recut_slow_apply), which only happens while the
// map is first built.
constexpr int kApplyThreads = 1024;
constexpr int kApplySub = kApplyThreads;  // subdividing leaves per level (one lane each)

// visit one worklist entry; returns children / candidate / subdivide flags
__device__ __forceinline__ void recut_visit_node(int node, const MP& mp, DevMap& m, int* kids, int& nchild,
                                                 int& is_cand, int& is_sub) {
  nchild = 0;
  is_cand = 0;
  is_sub = 0;
  if (node < 0) return;
  NodeHdr& h = m.hdr[node];
  if (h.octo == 1) {
    for (int o = 0; o < 8; o++)
      if (h.child[o] >= 0) kids[nchild++] = h.child[o];
    return;
  }
  h.opt_state = -1;
  const Clu& a = m.pcr_add[node];
  if (a.N <= mp.minpt[h.layer]) {
    h.is_plane = 0;
  } else if (h.isexist && h.has_sw) {
    V3 ev;
    M3 U;
    eig3(clu_cov(a), ev, U);
    double* e = &m.eig[(size_t)node * 12];
    for (int j = 0; j < 3; j++) e[j] = ev[j];
    for (int j = 0; j < 9; j++) e[3 + j] = U[j];
    h.is_plane = (ev[0] < mp.min_eig && (ev[0] / ev[2]) < mp.thre[h.layer]) ? 1 : 0;
    if (h.is_plane) {
      is_cand = !(ev[0] / ev[1] > 0.12) ? 1 : 0;  // tras_opt filter, octree.cpp:502-505
    } else if (h.layer < mp.max_layer) {
      m.nscr[(size_t)node * 4 + 2] = 1;  // subdividing
      is_sub = 1;
    }
  }
}

__global__ void __launch_bounds__(256) k_rc_visit(int L, int thread_num, const int* __restrict__ work_in, MP mp,
                                                  DevMap m, int* __restrict__ next, int* __restrict__ sub,
                                                  int* __restrict__ cand, int* __restrict__ rc,
                                                  uint32_t* __restrict__ cand_bits) {
  if (rc[kRcAbort]) return;
  const int nw = (L == 0) ? m.counters[kCntSlide] : rc[kRcLvl + L - 1];
  if (L == 0 && g_slide(m) < thread_num) return;  // local_mapping.cpp:150-154 (global count)
  const int* work = (L == 0) ? m.slide : work_in;
  for (int base = blockIdx.x * blockDim.x; base < nw; base += gridDim.x * blockDim.x) {
    const int q = base + threadIdx.x;
    int kids[8], nchild, is_cand, is_sub;
    recut_visit_node(q < nw ? work[q] : -1, mp, m, kids, nchild, is_cand, is_sub);
    const int node = q < nw ? work[q] : -1;
    int o1, o2, o3;
    wave_append3(&rc[kRcLvl + L], nchild, &m.counters[kCntFactors], is_cand, &rc[kRcSub + L], is_sub, o1, o2, o3);
    for (int j = 0; j < nchild; j++) next[o1 + j] = kids[j];
    if (is_cand) {
      cand[o2] = node;
      if (cand_bits) atomicOr(&cand_bits[node >> 5], 1u << (node & 31));  // k_fac_sort's id order
    }
    if (is_sub) sub[o3] = node;
  }
}

// The points of every subdividing leaf (subdivide / fix_divide, octree.cpp:
// 257-300), one wave per leaf: its point_fix list, then its run of each
// window slot (DevMap::lseg) in frame order. Pass 1 finds each point's octant
// and counts per octant; pass 2 writes the events of each octant into their
// own range of the leaf's block of the event list, in walk order, so a child's
// events come out grouped and already in the reference's push order (point_fix
// by index, then frame by frame, index ascending) — no sort. Event: phase << 21
// | index (phase 0 point_fix, 1 + ord a window frame). rcinfo[18 q ..]: the
// block's start, then per octant its offset and count, then the mask of
// non-empty octants; nscr[leaf*4+0] = q.
constexpr int kRcWinWaves = 4;
constexpr int kRcWalkB = 4;  // rc_win_leaf: 64-point chunks per round of loads
constexpr int kRcInfo = 18;  // event base, 8 octant offsets, 8 octant counts, octant mask
// one wave per subdividing leaf: the leaf's points are flattened across the
// phases so each 64-point chunk costs one round of loads whatever the runs'
// lengths; pass 1 counts the octants, pass 2 writes each octant's events
// (ph << 21 | idx) at its running position, walk order kept. The leaf's
// children-to-be are counted into rc[kRcNch + L] (the fused level kernel
// sizes its pushes from it).
__device__ __forceinline__ void rc_win_leaf(int L, int leaf, int q, const WinD* __restrict__ win, DevMap& m,
                                            uint64_t* __restrict__ ev, int* __restrict__ rcinfo, int cap,
                                            int info_cap, int* __restrict__ rc) {
  const int lane = threadIdx.x & 63;
#ifdef VG_PROBE
  const unsigned long long wl_t0 = wall_clock64();  // scripts/probe_recut.py: 16-20 split time / points
#endif
  const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const int wc = win->win_count;
  const int mp_l = win->mp[lane >= 1 && lane <= 32 ? lane - 1 : 0];  // in the same round of loads as wc
  const int my_slot = (lane >= 1 && lane <= wc) ? mp_l : 0;
  const NodeHdr& h = m.hdr[leaf];
  int len = 0, st = 0;
  if (lane == 0) len = h.fix_cnt;
  else if (lane <= wc && !lseg_get(m, leaf, my_slot, st, len)) len = 0;
  int ex = len;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(ex, off, 64);
    if (lane >= off) ex += y;
  }
  const int total = __shfl(ex, 63, 64);
  ex -= len;
  int base = 0;
  if (lane == 0) base = atomicAdd(&rc[kRcWin + L], total);
  base = __shfl(base, 0, 64);
  if ((size_t)q * kRcInfo + kRcInfo > (size_t)info_cap || base + total > cap) {
    if (lane == 0) {
      atomicOr(&m.counters[kCntErr], 16);
      if ((size_t)q * kRcInfo + kRcInfo <= (size_t)info_cap) rcinfo[(size_t)q * kRcInfo + 17] = 0;  // no children
    }
    return;
  }
  // kRcWalkB chunks of 64 walk points per round of loads (the index loads of
  // all of them, then all their point loads): a split costs two memory round
  // trips per batch instead of two per chunk; a leaf of at most one batch
  // keeps it in registers for pass 2
  constexpr int kB = kRcWalkB;
  int bph[kB], bix[kB], boc[kB];
  auto walk_batch = [&](int c0) __attribute__((always_inline)) {
    int loc[kB], pst[kB], psl[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) {
      const int e = min((c0 + b) * 64 + lane, total - 1);
      int ph = 0;
#pragma unroll
      for (int step = 32; step >= 1; step >>= 1) {
        const int cand = ph + step;
        const int v = __shfl(ex, cand <= wc ? cand : wc, 64);
        if (cand <= wc && v <= e) ph = cand;
      }
      bph[b] = ph;
      loc[b] = e - __shfl(ex, ph, 64);
      pst[b] = __shfl(st, ph, 64);
      psl[b] = __shfl(my_slot, ph, 64);
      bix[b] = ph == 0 ? loc[b] : m.wp_ord[(size_t)psl[b] * m.ord_stride + pst[b] + loc[b]];
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      const int ph = bph[b];
      const V3 pw = ph == 0 ? ld_v3(&m.fix_pnt[((size_t)h.fix_off + loc[b]) * 3])
                            : rigid(ld_m3(win->R[ph - 1]), ld_v3(&m.wp_pnt[((size_t)psl[b] * m.cap_wp + bix[b]) * 3]),
                                    ld_v3(win->p[ph - 1]));
      boc[b] = octant(pw, h.center);
    }
  };
  int cnt8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c0 = 0; c0 * 64 < total; c0 += kB) {
    walk_batch(c0);
#pragma unroll
    for (int b = 0; b < kB; b++) {
      const int e = (c0 + b) * 64 + lane;
      int o = boc[b];
      if (e < total) m.cfirst[(size_t)leaf * 8 + o] = -5;
      else o = -1;
#pragma unroll
      for (int k = 0; k < 8; k++) cnt8[k] += __popcll(__ballot(o == k));
    }
  }
  int off8[8], run = 0, mask = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    off8[k] = run;
    run += cnt8[k];
    mask |= (cnt8[k] > 0) << k;
  }
  if (lane == 0) {
    int* inf = rcinfo + (size_t)q * kRcInfo;
    inf[0] = base;
    for (int k = 0; k < 8; k++) {
      inf[1 + k] = off8[k];
      inf[9 + k] = cnt8[k];
    }
    inf[17] = mask;
    m.nscr[(size_t)leaf * 4 + 0] = q;
    atomicAdd(&rc[kRcNch + L], __popc(mask));
  }
  const bool kept = total <= 64 * kB;  // pass 1's only batch is still in registers
  for (int c0 = 0; c0 * 64 < total; c0 += kB) {
    if (!kept) walk_batch(c0);
#pragma unroll
    for (int b = 0; b < kB; b++) {
      const int e = (c0 + b) * 64 + lane;
      const int o = e < total ? boc[b] : -1;
      int pos = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint64_t bk = __ballot(o == k);
        if (o == k) pos = base + off8[k] + __popcll(bk & below);
        off8[k] += __popcll(bk);
      }
      if (o >= 0) ev[pos] = ((uint64_t)bph[b] << 21) | (uint64_t)bix[b];
    }
  }
#ifdef VG_PROBE
  if (lane == 0) {
    const unsigned long long d = wall_clock64() - wl_t0;
    atomicMax(&g_probe[16], d);
    atomicAdd(&g_probe[17], d);
    atomicAdd(&g_probe[18], 1ull);
    atomicMax(&g_probe[19], (unsigned long long)total);
    atomicAdd(&g_probe[20], (unsigned long long)total);
  }
#endif
}
__global__ void __launch_bounds__(64 * kRcWinWaves) k_rc_win(int L, const int* __restrict__ sub,
                                                             const WinD* __restrict__ win, DevMap m,
                                                             uint64_t* __restrict__ ev, int* __restrict__ rcinfo,
                                                             int cap, int info_cap, int* __restrict__ rc) {
  if (rc[kRcAbort]) return;
  const int nsub = rc[kRcSub + L];
  if (win->win_count > 63) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(&m.counters[kCntErr], 16);
    return;
  }
  for (int q = blockIdx.x * kRcWinWaves + (threadIdx.x >> 6); q < nsub; q += gridDim.x * kRcWinWaves)
    rc_win_leaf(L, sub[q], q, win, m, ev, rcinfo, cap, info_cap, rc);
}

// finish a subdivided parent: release its SlideWindow, free point_fix,
// octo_state = 1 (octree.cpp:375-387)
__device__ __forceinline__ void sub_finish(DevMap& m, int p) {
  NodeHdr& h = m.hdr[p];
  h.has_sw = 0;
  for (int j = 0; j < m.W; j++) clu_zero(m.pcrs[(size_t)p * m.W + j]);
  h.fix_cnt = 0;
  h.fix_cap = 0;
  h.octo = 1;
  m.nscr[(size_t)p * 4 + 2] = -1;
}

// one workgroup: the subdividing leaves in ascending id order (deterministic
// child ids), their marked octants' children allocated as one block (base +
// prefix), each child's event range from k_rc_win's per-octant blocks
// (cseg), the parents finished. More subdividing leaves than the workgroup's
// lanes (or than the test knob sub_cap) hand the level to the host-sized path.
__device__ __forceinline__ void rc_child_segs(const DevMap& m, int p, int c0, const int* __restrict__ rcinfo,
                                              int* __restrict__ cseg) {
  const int* inf = rcinfo + (size_t)m.nscr[(size_t)p * 4 + 0] * kRcInfo;
  int k = 0;
  for (int o = 0; o < 8; o++) {
    if (m.hdr[p].child[o] < 0 || inf[9 + o] == 0) continue;
    cseg[2 * (c0 + k)] = inf[0] + inf[1 + o];
    cseg[2 * (c0 + k) + 1] = inf[0] + inf[1 + o] + inf[9 + o];
    k++;
  }
}
__global__ void __launch_bounds__(kApplyThreads) k_rc_apply(int L, int sub_cap, DevMap m, int* __restrict__ next,
                                                            const int* __restrict__ sub,
                                                            const int* __restrict__ rcinfo, int* __restrict__ cseg,
                                                            int* __restrict__ rc) {
  __shared__ int s_sub[kApplySub];
  __shared__ int s_wsum[32];
  const int tid = threadIdx.x;
  if (rc[kRcAbort]) return;
  const int nsub = rc[kRcSub + L];
  if (nsub == 0) return;
  VG_PROBE_BEGIN();
  if (nsub > sub_cap) {
    if (tid == 0) rc[kRcAbort] = L + 1;
    return;
  }
  int myp = tid < nsub ? sub[tid] : 0x7fffffff;
  {  // rank among the level's leaves, read from LDS (ids are distinct)
    __shared__ __attribute__((aligned(16))) int s_in[kApplySub];
    s_in[tid] = myp;
    __syncthreads();
    int rank = 0;
    if (tid < nsub) {
      const int4* v4 = reinterpret_cast<const int4*>(s_in);
      for (int q = 0; q < (nsub + 3) / 4; q++) {
        const int4 v = v4[q];
        rank += (v.x < myp) + (v.y < myp) + (v.z < myp) + (v.w < myp);
      }
    }
    __syncthreads();
    if (tid < nsub) s_sub[rank] = myp;
  }
  __syncthreads();
  const int p_t = tid < nsub ? s_sub[tid] : -1;
  int cc = 0;
  if (p_t >= 0)
    for (int o = 0; o < 8; o++) cc += (m.cfirst[(size_t)p_t * 8 + o] == -5) ? 1 : 0;
  int ntot;
  const int coff = block_excl_scan(cc, s_wsum, &ntot);
  const int base = m.counters[kCntNodes];
  const int nnext = rc[kRcLvl + L];
  __syncthreads();
  if (p_t >= 0) {
    alloc_parent(m, p_t, base + coff, next, nnext + coff);
    rc_child_segs(m, p_t, coff, rcinfo, cseg);
  }
  __syncthreads();
  if (tid == 0) {
    m.counters[kCntNodes] = base + ntot;
    rc[kRcLvl + L] = nnext + ntot;
    rc[kRcCh + L] = ntot;
    rc[kRcChBase + L] = base;
  }
  if (p_t >= 0) sub_finish(m, p_t);
  VG_PROBE_MARK(17);
#ifdef VG_PROBE
  if (tid == 0) atomicAdd(&g_probe[62], 1ull);
#endif
}

constexpr int kRcPushWaves = 4;
constexpr int kPushScan = 4;    // event batches a push scans in one round (rc_push_child)
constexpr int kPreN = 32 * 9;   // s_pre: the frame clusters' P/v, then their point counts
constexpr int kPreV = 5;        // s_pre values per lane (32 slots * 10 / 64)
// the pushes of one child (push_fix then push per frame, octree.cpp:151-188)
// by one wave: its events keys[j0, j1) (point_fix first, then frame by
// frame), its parent and layer given (the caller may have initialised the
// header in this same wave); E / s_slot / s_pre: the wave's LDS slices. Role
// layout: 0-8 accumulated cluster, 9-17 fixed cluster (point_fix events),
// 18-62 cov_add, 63-71 the frame cluster of the current window slot (lanes
// 0-7 carry a second role)
__device__ __forceinline__ void rc_push_child(int child, int parent, int layer, int j0, int j1,
                                              const uint64_t* __restrict__ keys, const MP& mp,
                                              const WinD* __restrict__ win, DevMap& m, double (*E)[kErec],
                                              int* s_slot, double* s_pre, const RoleIdx& ri0, const RoleIdx& ri1) {
  const int lane = threadIdx.x & 63;
  const int r0 = lane, r1 = lane + 64;
  const bool has1 = r1 < 72;
  NodeHdr& h = m.hdr[child];
  const NodeHdr& ph = m.hdr[parent];
  const bool listed = layer < mp.max_layer;
#ifdef VG_PROBE
  const bool pr = blockIdx.x == 0 && threadIdx.x == 0;  // workgroup 0's wave 0: 40 pushes, 41 events,
  unsigned long long pt0 = wall_clock64();              // 42 prologue, 43 batch loads, 44 serial sums
  if (pr) {
    atomicAdd(&g_probe[40], 1ull);
    atomicAdd(&g_probe[41], (unsigned long long)(j1 - j0));
  }
#define PUSH_MARK(k)                                    \
  do {                                                  \
    if (pr) {                                           \
      const unsigned long long n_ = wall_clock64();     \
      atomicAdd(&g_probe[(k)], n_ - pt0);               \
      pt0 = n_;                                         \
    }                                                   \
  } while (0)
#else
#define PUSH_MARK(k) (void)0
#endif
  // the child's events are phase << 21 | index, ascending: point_fix
  // (phase 0) first, then one contiguous run per window slot (phase 1 + ord).
  // Up to kPushScan batches are read in one round of loads and the runs are
  // counted with ballots; longer children binary-search the keys.
  const int nev = j1 - j0, wc = listed ? win->win_count : 0;
  // the prologue's other loads go out with the keys' (one round): each
  // lane's window slot and its epoch, the frame clusters (s_pre, stored
  // below) and the accumulators' starting values
  const int mp_l = win->mp[lane < 32 ? lane : 0];  // in the same round of loads as win_count
  const int my_slot = lane < win->win_count ? mp_l : 0;  // listed or not (the batches read it)
  const int my_epoch = lane < wc ? m.slot_epoch[my_slot] : 0;
  double pv[kPreV];
#pragma unroll
  for (int i = 0; i < kPreV; i++) {
    const int t = lane + 64 * i;
    pv[i] = 0.0;
    if (t < mp.W * 10) {
      const int sl = t < mp.W * 9 ? t / 9 : t - mp.W * 9, q = t < mp.W * 9 ? t % 9 : 9;
      const Clu& lc = m.pcrs[(size_t)child * mp.W + sl];
      pv[i] = q < 6 ? lc.P[q] : (q < 9 ? lc.v[q - 6] : (double)lc.N);
    }
  }
  auto acc_ptr = [&](int r, int slot) -> double* {
    if (r < 9) return r < 6 ? &m.pcr_add[child].P[r] : &m.pcr_add[child].v[r - 6];
    if (r < 18) return r < 15 ? &m.pcr_fix[child].P[r - 9] : &m.pcr_fix[child].v[r - 15];
    if (r < 63) return &m.cov_add[(size_t)child * kCovN + r - 18];
    Clu& lc = m.pcrs[(size_t)child * mp.W + slot];
    return r < 69 ? &lc.P[r - 63] : &lc.v[r - 69];
  };
  double a0 = r0 < 63 ? *acc_ptr(r0, 0) : 0.0, a1 = 0.0;
  const int n_add0 = lane == 0 ? m.pcr_add[child].N : 0, n_fix0 = lane == 0 ? m.pcr_fix[child].N : 0;
  int nfix = 0, run_lo = 0, run_n = 0;
  const bool short_ev = nev <= 64 * kPushScan;  // the keys stay in registers (kv) for the batches below
  uint64_t kv[kPushScan];
  if (short_ev) {
    int phv[kPushScan];
#pragma unroll
    for (int b = 0; b < kPushScan; b++) {
      const int e = 64 * b + lane;
      kv[b] = e < nev ? keys[j0 + e] : 0ull;
      phv[b] = e < nev ? (int)((kv[b] >> 21) & 63) : 64;
    }
#pragma unroll
    for (int b = 0; b < kPushScan; b++) nfix += __popcll(__ballot(phv[b] == 0));
    for (int q = 1, acc = nfix; q <= wc && acc < nev; q++) {
      int c = 0;
#pragma unroll
      for (int b = 0; b < kPushScan; b++) c += __popcll(__ballot(phv[b] == q));
      if (lane == q - 1) {
        run_lo = j0 + acc;
        run_n = c;
      }
      acc += c;
    }
  } else {
    for (int b0 = j0; b0 < j1; b0 += 64) {
      const int e = b0 + lane;
      const bool f = e < j1 && ((keys[e] >> 21) & 63) == 0;
      const int k = __popcll(__ballot(f));
      nfix += k;
      if (k < 64) break;
    }
    if (lane < wc) {
      auto lower = [&](uint64_t key) {
        int lo = j0, hi = j1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (keys[mid] < key) lo = mid + 1;
          else hi = mid;
        }
        return lo;
      };
      run_lo = lower((uint64_t)(lane + 1) << 21);
      run_n = lower((uint64_t)(lane + 2) << 21) - run_lo;
    }
  }
  // the point_fix block and the slots' runs are allocated in one round (an
  // overflow of either fails the scan with VG_E_CAPACITY, so a run taken
  // beside a point_fix overflow is never used); the returning atomics are
  // consumed after the first batch's loads (settle), so their round trip
  // overlaps those loads
  int off = 0, run_st = 0;
  if (lane == 0 && nfix > 0 && listed) off = atomicAdd(&m.counters[kCntFix], nfix);
  if (lane < wc && run_n > 0) run_st = atomicAdd(&m.arena[my_slot], run_n);
  int fix_off = 0;
  bool settled = false;
  auto settle = [&]() __attribute__((always_inline)) {  // false: point_fix overflow (wave-uniform)
    settled = true;
    if (nfix > 0 && listed) {
      if (lane == 0) {
        if (off + nfix > m.cap_fix) {
          atomicOr(&m.counters[kCntErr], 8);
          off = -1;
        } else {
          h.fix_off = off;
          h.fix_cap = nfix;
          h.fix_cnt = nfix;
        }
      }
      fix_off = __shfl(off, 0, 64);
      if (fix_off < 0) return false;
    }
    // lane p < win_count holds phase p + 1's run in the slot's arena
    if (lane < wc && run_n > 0) {
      if (run_st + run_n > m.ord_stride) {
        atomicOr(&m.counters[kCntErr], 16);
        run_st = 0;
      } else {
        m.lseg[(size_t)child * mp.W + my_slot] = lseg_pack(run_st, run_n, my_epoch);
      }
    }
    // every slot's frame cluster, loaded above in one round (a slot's run is
    // contiguous, so each is read once, before this wave writes it): a
    // cluster switch then costs an LDS read, not a dependent HBM load; their
    // point counts sit at s_pre[kPreN + slot], so the count update at a
    // switch is a plain store
#pragma unroll
    for (int i = 0; i < kPreV; i++) {
      const int t = lane + 64 * i;
      if (t < mp.W * 10) s_pre[t < mp.W * 9 ? t : kPreN + t - mp.W * 9] = pv[i];
    }
    return true;
  };
  int cur_slot = -1, loc_n = 0, nwin = 0;
  PUSH_MARK(42);
  for (int b0 = j0; b0 < j1; b0 += 64) {
    const int e = b0 + lane, bi = (b0 - j0) >> 6;
    uint64_t k = 0ull;
    if (!short_ev) {
      k = e < j1 ? keys[e] : 0ull;
    } else {
#pragma unroll
      for (int b = 0; b < kPushScan; b++)  // (a register select: kv stays in VGPRs)
        if (bi == b) k = kv[b];
    }
    const int phase = (int)((k >> 21) & 63), idx = (int)(k & ((1u << 21) - 1));
    const int slot_e = __shfl(my_slot, phase > 0 ? phase - 1 : 0, 64);  // win->mp[phase - 1]
    V3 pt;
    M3 var;
    if (e < j1) {
      if (phase == 0) {
        const size_t f = (size_t)ph.fix_off + idx;
        pt = ld_v3(&m.fix_pnt[f * 3]);
        var = ld_m3(&m.fix_var[f * 9]);
        fill_record(E[lane], pt, pt, var);
        s_slot[lane] = -1;
      } else {
        const int ord = phase - 1, slot = slot_e;
        const size_t bb = (size_t)slot * m.cap_wp + idx;
        const V3 pnt = ld_v3(&m.wp_pnt[bb * 3]);
        fill_record(E[lane], pnt, rigid(ld_m3(win->R[ord]), pnt, ld_v3(win->p[ord])),
                    ld_m3(&m.wp_var[bb * 9]));
        s_slot[lane] = slot;
        m.wp_leaf[bb] = listed ? child : -1;
      }
    }
    if (!settled && !settle()) return;
    if (e < j1 && phase == 0 && listed) {  // the point_fix copy into the child's block
      const size_t d = (size_t)fix_off + (e - j0);
      for (int t = 0; t < 3; t++) m.fix_pnt[d * 3 + t] = pt[t];
      for (int t = 0; t < 9; t++) m.fix_var[d * 9 + t] = var[t];
    }
    if (listed) {  // the point into the child's run (ds_bpermute of the run's lane; uniform call)
      const int ph = e < j1 ? phase : 0;
      const int src = ph > 0 ? ph - 1 : 0;
      const int lo_p = __shfl(run_lo, src, 64), st_p = __shfl(run_st, src, 64);
      if (ph > 0) m.wp_ord[(size_t)slot_e * m.ord_stride + st_p + (e - lo_p)] = idx;
    }
    const int nb = (j1 - b0) < 64 ? (j1 - b0) : 64;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    PUSH_MARK(43);
#pragma unroll 4
    for (int k = 0; k < nb; k++) {
      const int slot = s_slot[k];
      const bool isfix = slot < 0;
      if (!isfix && slot != cur_slot) {  // frame cluster switch (uniform)
        if (cur_slot >= 0) {
          if (r0 >= 63) *acc_ptr(r0, cur_slot) = a0;
          if (has1) *acc_ptr(r1, cur_slot) = a1;
          if (lane == 63) m.pcrs[(size_t)child * mp.W + cur_slot].N = (int)s_pre[kPreN + cur_slot] + loc_n;
        }
        cur_slot = slot;
        if (r0 >= 63) a0 = s_pre[cur_slot * 9 + r0 - 63];
        if (has1) a1 = s_pre[cur_slot * 9 + r1 - 63];
        loc_n = 0;
      }
      const double* Ek = E[k];
      const bool use0 = r0 < 9 || (r0 >= 18 && r0 < 63) || (r0 < 18 ? isfix : !isfix);
      const double i0 = role_inc(Ek, ri0);
      if (use0) a0 += i0;
      if (has1 && !isfix) a1 += role_inc(Ek, ri1);
      if (!isfix) {
        loc_n++;
        nwin++;
      }
    }
    __builtin_amdgcn_wave_barrier();
    PUSH_MARK(44);
  }
#undef PUSH_MARK
  if (!settled && !settle()) return;  // no events
  if (r0 < 63) *acc_ptr(r0, 0) = a0;
  if (cur_slot >= 0) {
    if (r0 >= 63) *acc_ptr(r0, cur_slot) = a0;
    if (has1) *acc_ptr(r1, cur_slot) = a1;
    if (lane == 63) m.pcrs[(size_t)child * mp.W + cur_slot].N = (int)s_pre[kPreN + cur_slot] + loc_n;
  }
  if (lane == 0) {
    m.pcr_add[child].N = n_add0 + nev;
    m.pcr_fix[child].N = n_fix0 + nfix;
    if (nwin > 0) {
      h.has_sw = 1;
      h.isexist = 1;
    }
  }
}
__device__ __forceinline__ RoleIdx rc_push_role(int r) {
  if (r < 9) return role_clu(r, kEp);
  if (r < 18) return role_clu(r - 9, kEp);
  if (r < 63) return role_cov(r - 18);
  return role_clu(r - 63, kEq);
}

// pushes of one level's children, one wave per child (rc_push_child)
__global__ void __launch_bounds__(64 * kRcPushWaves) k_rc_push(int L, const uint64_t* __restrict__ keys,
                                                               const int* __restrict__ cseg, MP mp,
                                                               const WinD* __restrict__ win, DevMap m,
                                                               const int* __restrict__ rc) {
  __shared__ double E[kRcPushWaves][64][kErec];
  __shared__ int s_slot[kRcPushWaves][64];  // window slot of the event, -1 for point_fix
  __shared__ double s_pre[kRcPushWaves][32 * 10];  // the child's frame clusters, read ahead
  if (rc[kRcAbort]) return;
  const int nch = rc[kRcCh + L], cbase = rc[kRcChBase + L];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const RoleIdx ri0 = rc_push_role(lane), ri1 = rc_push_role(lane + 64 < 72 ? lane + 64 : 0);
  for (int c = blockIdx.x * kRcPushWaves + wv; c < nch; c += gridDim.x * kRcPushWaves) {
    const int child = cbase + c;
    const NodeHdr& h = m.hdr[child];
    rc_push_child(child, h.parent, h.layer, cseg[2 * c], cseg[2 * c + 1], keys, mp, win, m, E[wv], s_slot[wv],
                  s_pre[wv], ri0, ri1);
  }
}

// ---- the fused recut levels -------------------------------------------
// The level loop above costs four dependent launches per level (visit, win,
// apply, push). The fused form runs one launch per level boundary:
//   k_rc_level0   visit(0) + win(0): the slide roots, 64 per wave; each wave
//                 then splits the subdividing leaves its lanes found;
//   k_rc_level(L) apply(L) + push(L) + visit(L+1) + win(L+1): the level's
//                 subdividing leaves are sorted and their children counted in
//                 LDS by every workgroup that pushes (redundantly: the same
//                 ids k_rc_apply hands out, base + prefix in ascending parent
//                 id order, so node ids and every order derived from them are
//                 unchanged); one wave per child initialises it, pushes its
//                 events, visits it and, when it subdivides, splits its
//                 points for level L+1; the grid's last waves visit (and
//                 split) the level's other nodes, the children of internal
//                 nodes listed by visit(L).
// Level L's sub list / rcinfo / events and level L+1's live in alternate
// buffers (sub_of / info_of / ev_of), so one launch reads the first and
// writes the second. The node counter's value before the level is carried in
// rc (kRcNode0, then kRcChBase + kRcCh of the previous level), so no
// workgroup reads a counter another one advances. Abort and overflow
// semantics are the level loop's (rc[kRcAbort] = L + 1; the host-sized path
// replays from there).

// one wave: visit the list entries [64 j, 64 j + 64) of level L; appends the
// internal nodes' children to next, the candidates, the subdividing leaves
// to sub; then (do_win) splits each subdividing leaf (rc_win_leaf)
__device__ __forceinline__ void rc_visit_chunk(int L, const int* __restrict__ work, int nw, int j, const MP& mp,
                                               DevMap& m, int* __restrict__ next, int* __restrict__ sub,
                                               int* __restrict__ cand, int* __restrict__ rc,
                                               uint32_t* __restrict__ cand_bits, bool do_win,
                                               const WinD* __restrict__ win, uint64_t* __restrict__ ev,
                                               int* __restrict__ rcinfo, int cap) {
  const int q = j * 64 + (threadIdx.x & 63);
  const int node = q < nw ? work[q] : -1;
  int kids[8], nchild, is_cand, is_sub;
  recut_visit_node(node, mp, m, kids, nchild, is_cand, is_sub);
  int o1, o2, o3;
  wave_append3(&rc[kRcLvl + L], nchild, &m.counters[kCntFactors], is_cand, &rc[kRcSub + L], is_sub, o1, o2, o3);
  for (int k = 0; k < nchild; k++) next[o1 + k] = kids[k];
  if (is_cand) {
    cand[o2] = node;
    if (cand_bits) atomicOr(&cand_bits[node >> 5], 1u << (node & 31));  // k_fac_sort's id order
  }
  if (is_sub) sub[o3] = node;
  if (!do_win) return;
  uint64_t bs = __ballot(is_sub);
  while (bs) {
    const int l = __ffsll((unsigned long long)bs) - 1;
    bs &= bs - 1;
    rc_win_leaf(L, __shfl(node, l, 64), __shfl(o3, l, 64), win, m, ev, rcinfo, cap, cap, rc);
  }
}

constexpr int kRcFusedWaves = 4;
// in-kernel clock of the recut's level kernels (KClock rc_*, vg_profile bit 2)
__device__ __forceinline__ void rc_clock_start(KClock* clk) {
  if (clk && clk->on && blockIdx.x == 0 && threadIdx.x == 0) {
    const int slot = clk->scan & (kClkRcScans - 1);
    clk->rc_t0[slot] = (unsigned long long)wall_clock64();
    clk->rc_exec[slot] = 1;
  }
}
__device__ __forceinline__ void rc_clock_end(KClock* clk) {
  if (clk && clk->on && blockIdx.x < kClkRcBlocks) {
    __syncthreads();
    if (threadIdx.x == 0) clk->rc_tend[clk->scan & (kClkRcScans - 1)][blockIdx.x] = (unsigned long long)wall_clock64();
  }
}
__device__ __forceinline__ void rc_level0_body(int thread_num, const MP& mp, DevMap& m, int* __restrict__ next,
                                               int* __restrict__ sub, int* __restrict__ cand, int* __restrict__ rc,
                                               uint32_t* __restrict__ cand_bits, const WinD* __restrict__ win,
                                               uint64_t* __restrict__ ev, int* __restrict__ rcinfo, int cap);
// clk_end: this launch ends the scan's recut levels (max_layer 0)
__global__ void __launch_bounds__(64 * kRcFusedWaves) k_rc_level0(int thread_num, MP mp, DevMap m,
                                                                  int* __restrict__ next, int* __restrict__ sub,
                                                                  int* __restrict__ cand, int* __restrict__ rc,
                                                                  uint32_t* __restrict__ cand_bits,
                                                                  const WinD* __restrict__ win,
                                                                  uint64_t* __restrict__ ev,
                                                                  int* __restrict__ rcinfo, int cap, KClock* clk,
                                                                  int clk_end) {
  rc_clock_start(clk);
  rc_level0_body(thread_num, mp, m, next, sub, cand, rc, cand_bits, win, ev, rcinfo, cap);
  if (clk_end) rc_clock_end(clk);
}
__device__ __forceinline__ void rc_level0_body(int thread_num, const MP& mp, DevMap& m, int* __restrict__ next,
                                               int* __restrict__ sub, int* __restrict__ cand, int* __restrict__ rc,
                                               uint32_t* __restrict__ cand_bits, const WinD* __restrict__ win,
                                               uint64_t* __restrict__ ev, int* __restrict__ rcinfo, int cap) {
  if (blockIdx.x == 0 && threadIdx.x == 0) rc[kRcNode0] = m.counters[kCntNodes];  // k_rc_level(0)'s id base
  if (rc[kRcAbort]) return;
  if (g_slide(m) < thread_num) return;  // local_mapping.cpp:150-154 (global count)
  const int nw = m.counters[kCntSlide];
  const bool wide = win->win_count > 63;
  if (wide && mp.max_layer > 0) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(&m.counters[kCntErr], 16);
  }
  const bool do_win = mp.max_layer > 0 && !wide;
  const int nwv = gridDim.x * kRcFusedWaves;
  for (int j = blockIdx.x * kRcFusedWaves + (threadIdx.x >> 6); j * 64 < nw; j += nwv)
    rc_visit_chunk(0, m.slide, nw, j, mp, m, next, sub, cand, rc, cand_bits, do_win, win, ev, rcinfo, cap);
}

__device__ __forceinline__ void rc_level_body(
    int L, int sub_cap, const MP& mp, DevMap& m, const int* __restrict__ sub_in, const int* __restrict__ info_in,
    const uint64_t* __restrict__ ev_in, int* __restrict__ next, int* __restrict__ next2, int* __restrict__ sub_out,
    int* __restrict__ cand, int* __restrict__ rc, uint32_t* __restrict__ cand_bits, const WinD* __restrict__ win,
    uint64_t* __restrict__ ev_out, int* __restrict__ info_out, int cap);
// clk_end: the scan's last level kernel (its workgroups stamp the recut's end)
__global__ void __launch_bounds__(64 * kRcFusedWaves) k_rc_level(
    int L, int sub_cap, MP mp, DevMap m, const int* __restrict__ sub_in, const int* __restrict__ info_in,
    const uint64_t* __restrict__ ev_in, int* __restrict__ next, int* __restrict__ next2, int* __restrict__ sub_out,
    int* __restrict__ cand, int* __restrict__ rc, uint32_t* __restrict__ cand_bits, const WinD* __restrict__ win,
    uint64_t* __restrict__ ev_out, int* __restrict__ info_out, int cap, KClock* clk, int clk_end) {
  rc_level_body(L, sub_cap, mp, m, sub_in, info_in, ev_in, next, next2, sub_out, cand, rc, cand_bits, win, ev_out,
                info_out, cap);
  if (clk_end) rc_clock_end(clk);
}
__device__ __forceinline__ void rc_level_body(
    int L, int sub_cap, const MP& mp, DevMap& m, const int* __restrict__ sub_in, const int* __restrict__ info_in,
    const uint64_t* __restrict__ ev_in, int* __restrict__ next, int* __restrict__ next2, int* __restrict__ sub_out,
    int* __restrict__ cand, int* __restrict__ rc, uint32_t* __restrict__ cand_bits, const WinD* __restrict__ win,
    uint64_t* __restrict__ ev_out, int* __restrict__ info_out, int cap) {
  __shared__ __attribute__((aligned(16))) int s_in[kApplySub];
  __shared__ int s_sub[kApplySub], s_q[kApplySub], s_mask[kApplySub], s_coff[kApplySub];
  __shared__ int s_ws[kRcFusedWaves];
  __shared__ double E[kRcFusedWaves][64][kErec];
  __shared__ int s_slot[kRcFusedWaves][64];
  __shared__ double s_pre[kRcFusedWaves][32 * 10];
  if (rc[kRcAbort]) return;
  const int nsub = rc[kRcSub + L];
  if (nsub > sub_cap) {  // the host-sized path replays from this level
    if (blockIdx.x == 0 && threadIdx.x == 0) rc[kRcAbort] = L + 1;
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ntot = rc[kRcNch + L];  // children of this level's subdividing leaves (rc_win_leaf)
  const int A = rc[kRcLvl + L];     // level L+1's other nodes (visit(L))
#ifdef VG_PROBE
  const int pb = L < 2 ? 8 * L : 32;  // per level: calls, sort, prefix, push, tail, nsub, ntot, A (block 0)
  VG_PROBE_BEGIN();
  if (blockIdx.x == 0 && tid == 0 && L < 3) {
    atomicAdd(&g_probe[pb], 1ull);
    atomicAdd(&g_probe[pb + 5], (unsigned long long)nsub);
    atomicAdd(&g_probe[pb + 6], (unsigned long long)ntot);
    atomicAdd(&g_probe[pb + 7], (unsigned long long)A);
  }
#define RC_MARK(k) \
  do {             \
    if (blockIdx.x == 0 && L < 3) VG_PROBE_MARK(pb + (k)); \
  } while (0)
#else
#define RC_MARK(k) (void)0
#endif
  const int base = (L == 0) ? rc[kRcNode0] : rc[kRcChBase + L - 1] + rc[kRcCh + L - 1];
  if (blockIdx.x == 0 && tid == 0) {
    rc[kRcCh + L] = ntot;
    rc[kRcChBase + L] = base;
    rc[kRcTot + L] = A + ntot;
    m.counters[kCntNodes] = base + ntot;
  }
  const bool wide = win->win_count > 63;
  const bool do_win = (L + 1 < mp.max_layer) && !wide;
  if (wide && L + 1 < mp.max_layer && blockIdx.x == 0 && tid == 0) atomicOr(&m.counters[kCntErr], 16);
  // every subdividing leaf becomes internal (alloc_parent's mark, sub_finish), children or not; the
  // pushes below read only the parents' fix_off and geometry, which this leaves alone
  for (int i = blockIdx.x * blockDim.x + tid; i < nsub; i += gridDim.x * blockDim.x) {
    const int p = sub_in[i];
    m.nscr[(size_t)p * 4 + 1] = -1;
    sub_finish(m, p);
  }
  if ((int)blockIdx.x * kRcFusedWaves < ntot) {
    // apply(L): the subdividing leaves in ascending id order (rank among distinct ids, from LDS),
    // each with its rcinfo slot (its index in sub_in, rc_win_leaf's q) and octant mask, read in
    // the same round as the ids
    constexpr int kPer = kApplySub / (64 * kRcFusedWaves);
    int mk_t[kPer];
#pragma unroll
    for (int k = 0; k < kPer; k++) {
      const int t = tid + k * 64 * kRcFusedWaves;
      s_in[t] = t < nsub ? sub_in[t] : 0x7fffffff;
      mk_t[k] = (t < nsub && (size_t)t * kRcInfo + kRcInfo <= (size_t)cap) ? info_in[(size_t)t * kRcInfo + 17] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; k++) {
      const int t = tid + k * 64 * kRcFusedWaves;
      if (t >= nsub) break;
      const int myp = s_in[t];
      int rank = 0;
      const int4* v4 = reinterpret_cast<const int4*>(s_in);
      for (int u = 0; u < (nsub + 3) / 4; u++) {
        const int4 v = v4[u];
        rank += (v.x < myp) + (v.y < myp) + (v.z < myp) + (v.w < myp);
      }
      s_sub[rank] = myp;
      s_q[rank] = t;
      s_mask[rank] = mk_t[k];
    }
    __syncthreads();
    RC_MARK(1);
    // per parent: its rcinfo slot and non-empty octants; exclusive prefix of their counts (4 per thread)
    int c4[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int t = 4 * tid + k;
      c4[k] = 0;
      if (t < nsub) c4[k] = __popc(s_mask[t]);
      sum += c4[k];
    }
    int x = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    if (lane == 63) s_ws[wv] = x;
    __syncthreads();
    int run = x - sum;
    for (int k = 0; k < wv; k++) run += s_ws[k];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int t = 4 * tid + k;
      if (t < nsub) s_coff[t] = run;
      run += c4[k];
    }
    __syncthreads();
    RC_MARK(2);
    const RoleIdx ri0 = rc_push_role(lane), ri1 = rc_push_role(lane + 64 < 72 ? lane + 64 : 0);
    for (int c = blockIdx.x * kRcFusedWaves + wv; c < ntot; c += gridDim.x * kRcFusedWaves) {
      int lo = 0, hi = nsub - 1;  // the parent: the last t with s_coff[t] <= c
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_coff[mid] <= c) lo = mid;
        else hi = mid - 1;
      }
      const int t = lo, p = s_sub[t], k = c - s_coff[t];
      int mk = s_mask[t];
      for (int i = 0; i < k; i++) mk &= mk - 1;
      const int o = __ffs(mk) - 1;  // the parent's k-th non-empty octant
      if (o < 0) continue;
#ifdef VG_PROBE
      unsigned long long qt = wall_clock64();  // workgroup 0's wave 0: 48 init, 49 push, 51 visit, 52 win, 53 wins
      const bool qpr = blockIdx.x == 0 && tid == 0;
#define Q_MARK(k)                                   \
  do {                                              \
    if (qpr) {                                      \
      const unsigned long long n_ = wall_clock64(); \
      atomicAdd(&g_probe[(k)], n_ - qt);            \
      qt = n_;                                      \
    }                                               \
  } while (0)
#else
#define Q_MARK(k) (void)0
#endif
      const int* inf = info_in + (size_t)s_q[t] * kRcInfo;
      const int j0 = inf[0] + inf[1 + o], j1 = j0 + inf[9 + o];
      const int child = base + c;
      if (child >= m.cap_nodes) {
        if (lane == 0) atomicOr(&m.counters[kCntErr], 4);
        continue;
      }
      NodeHdr& ph = m.hdr[p];
      const int layer = ph.layer + 1;
      if (lane == 0) {  // alloc_parent for this octant
        const int xyz[3] = {(o >> 2) & 1, (o >> 1) & 1, o & 1};
        double cc[3];
        for (int jj = 0; jj < 3; jj++) cc[jj] = ph.center[jj] + (float)((2 * xyz[jj] - 1) * ph.qlen);
        init_node(m.hdr[child], cc, ph.qlen / 2, layer, p);
        dbox_child(m.dbox + (size_t)child * 6, m.dbox + (size_t)p * 6, ph.center, o);
        ph.child[o] = child;
        m.cfirst[(size_t)p * 8 + o] = 0x7f7f7f7f;
        next[A + c] = child;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      Q_MARK(48);
      rc_push_child(child, p, layer, j0, j1, ev_in, mp, win, m, E[wv], s_slot[wv], s_pre[wv], ri0, ri1);
      Q_MARK(49);
      // visit(L+1) of the new child (its cluster, counts and flags: this wave's stores just above)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      int kids[8], nchild, is_cand, is_sub;
      recut_visit_node(lane == 0 ? child : -1, mp, m, kids, nchild, is_cand, is_sub);
      int o1, o2, o3;
      wave_append3(&rc[kRcLvl + L + 1], 0, &m.counters[kCntFactors], is_cand, &rc[kRcSub + L + 1], is_sub, o1, o2,
                   o3);
      if (is_cand) {
        cand[o2] = child;
        if (cand_bits) atomicOr(&cand_bits[child >> 5], 1u << (child & 31));
      }
      if (is_sub) sub_out[o3] = child;
      Q_MARK(51);
      if (do_win && __shfl(is_sub, 0, 64)) {
        rc_win_leaf(L + 1, child, __shfl(o3, 0, 64), win, m, ev_out, info_out, cap, cap, rc);
#ifdef VG_PROBE
        if (qpr) atomicAdd(&g_probe[53], 1ull);
#endif
      }
      Q_MARK(52);
#undef Q_MARK
    }
    RC_MARK(3);
  }
  // visit(L+1) (+ win(L+1)) of the level's other nodes, from the grid's last waves
  const int nwv = gridDim.x * kRcFusedWaves;
  for (int j = nwv - 1 - ((int)blockIdx.x * kRcFusedWaves + wv); j * 64 < A; j += nwv)
    rc_visit_chunk(L + 1, next, A, j, mp, m, next2, sub_out, cand, rc, cand_bits, do_win, win, ev_out, info_out, cap);
  RC_MARK(4);
#undef RC_MARK
}

// ---- host-sized path (overflow replay) ----------------------------------
// the children's event ranges of the sorted parents (ids c0 + prefix, as
// alloc_children handed them out)
__global__ void __launch_bounds__(256) k_sub_cseg(int ns, const int* __restrict__ sub, const uint32_t* __restrict__ off,
                                                  DevMap m, const int* __restrict__ rcinfo, int* __restrict__ cseg) {
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < ns; q += gridDim.x * blockDim.x)
    rc_child_segs(m, sub[q], (int)off[q], rcinfo, cseg);
}
__global__ void __launch_bounds__(256) k_sub_finish(int ns, const int* __restrict__ sub, DevMap m) {
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < ns; q += gridDim.x * blockDim.x) sub_finish(m, sub[q]);
}

// tras_opt: factor list in node-id order; opt_state = factor index
__global__ void __launch_bounds__(256) k_factor_finish(int nf, const int* __restrict__ fac, DevMap m, int* __restrict__ fac_node,
                                double* __restrict__ fac_eig, Clu* __restrict__ fac_pcr) {
  for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < nf; a += gridDim.x * blockDim.x) {
    int node = fac[a];
    fac_node[a] = node;
    m.hdr[node].opt_state = a;
    for (int j = 0; j < 12; j++) fac_eig[(size_t)a * 12 + j] = m.eig[(size_t)node * 12 + j];
    fac_pcr[a] = m.pcr_add[node];
  }
}

// a recut level's subdividing leaves, rcinfo and events (alternate buffers per level)
static int* sub_of(Work& w, int L) { return (L % 2 == 0) ? w.list2 : w.sub_odd; }
static int* info_of(Work& w, int L) { return (L % 2 == 0) ? (int*)w.v1 : w.info_odd; }
static uint64_t* ev_of(Work& w, int L) { return (L % 2 == 0) ? w.k0 : w.ev_odd; }

static int read_rc(vg_ctx* ctx, int* h) {
  VG_HIP(hipMemcpyAsync(h, ctx->wk.rc, kRcN * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  return read_counters(ctx);  // synchronizes
}

// host-sized apply of level L (k_rc_visit and k_rc_win already ran): sorted
// subdividing leaves, host-sized child allocation, the children's event
// ranges, then the device pushes (k_rc_push) and the parents' finish
static int recut_slow_apply(vg_ctx* ctx, int L, const MP& mp, WinD* dwin, int* next, int* hrc) {
  DevMap& m = ctx->map;
  Work& w = ctx->wk;
  hipStream_t s = ctx->stream;
  const int nsub = hrc[kRcSub + L], nnext = hrc[kRcLvl + L];
  if (nsub <= 0) return VG_OK;
  int* sub = sub_of(w, L);
  VG_TRY(sort_ids_inplace(ctx, sub, nsub));
  VG_TRY(read_counters(ctx));
  const int first = ctx->h_pinned[kCntNodes];
  int created = 0;
  VG_TRY(alloc_children(ctx, sub, nsub, next, nnext, true, &created));
  k_sub_cseg<<<grid_for(nsub), kBlock, 0, s>>>(nsub, sub, w.ac_off, m, info_of(w, L), (int*)w.ac_cnt);
  VG_HIP(hipMemsetD32Async((hipDeviceptr_t)(w.rc + kRcLvl + L), nnext + created, 1, s));
  VG_HIP(hipMemsetD32Async((hipDeviceptr_t)(w.rc + kRcCh + L), created, 1, s));
  VG_HIP(hipMemsetD32Async((hipDeviceptr_t)(w.rc + kRcChBase + L), first, 1, s));
  k_rc_push<<<256, 64 * kRcPushWaves, 0, s>>>(L, ev_of(w, L), (const int*)w.ac_cnt, mp, dwin, m, w.rc);
  k_sub_finish<<<grid_for(nsub), kBlock, 0, s>>>(nsub, sub, m);
  VG_HIP(hipGetLastError());
  return read_counters(ctx);
}

// the recut's head as one launch: the window view (poses from the device
// state, ring, per-ord counts), then the level counters cleared
__global__ void k_make_win_recut_begin(DState* __restrict__ st, WinArg wa, const int* __restrict__ wpn,
                                       WinD* __restrict__ win, int* __restrict__ nper, int* __restrict__ slot_of,
                                       DevMap m, int* __restrict__ rc, int thread_num) {
  make_win_block(st, wa, wpn, win, nper, slot_of);
  __syncthreads();
  recut_begin_block(m, rc, thread_num);
}

// Asynchronous factor extraction (tras_opt, octree.cpp:491-516) sized on the
// device. k_rc_visit marks every candidate in a bitmap over node ids; one
// workgroup turns the bitmap into the id-ascending factor list (the host
// path's sort order) with one prefix sum over the allocated id range, clearing
// it as it reads, then k_factor_finish_dev fills the factor arrays. k_fac_sort
// also publishes the recut status and the factor count (Pub::seq_rc) and
// leaves the status in rc[kRcStatus], where k_ba_init reads it: a recut that
// needs the host-sized path (insert replay, level overflow, more factors than
// max_fac) makes the LM skip, and the host completes the recut and reruns it.
// xa.frame (sharded): the status goes out in the exchange frame (site 5),
// closed here; k_pub_rc takes the sum
__global__ void __launch_bounds__(1024) k_fac_sort(DevMap m, int* __restrict__ rc, uint32_t* __restrict__ bits,
                                                   int* __restrict__ fac_node, int cap_f, Pub* __restrict__ pub,
                                                   int* __restrict__ seq_ctr, int max_fac, XchgArg xa) {
  fac_sort_block(m, rc, bits, fac_node, cap_f, pub, seq_ctr, max_fac, xa.frame == nullptr);
  if (xa.frame) {
    for (int i = threadIdx.x + 1; i < xa.n - 2; i += blockDim.x) xa.frame[i] = 0.0;
    if (threadIdx.x == 0) {  // (fac_sort_block's thread 0 wrote rc[kRcStatus])
      xa.frame[0] = (double)rc[kRcStatus];
      xchg_close(xa.frame, xa.n, 5, xa.seq);
    }
  }
}
// sharded mode: the recut status summed over the ranks into rc[kRcStatus], so
// every rank's k_ba_init skips alike and every host takes the same host-sized
// completion and LM rerun — the ranks' exchange sequences stay in step (a
// guard mismatch: error bit 32, VG_E_STATE with the scan's counters). The
// factor count published is this rank's own.
__global__ void k_pub_rc(const DevMap m, int* __restrict__ rc, Pub* __restrict__ pub, const int* __restrict__ seq_ctr,
                         XchgArg xa) {
  if (threadIdx.x == 0) {
    const bool ok = xchg_ok(xa.frame, xa.n, xa.world);
    if (!ok) atomicOr(xa.err, 32);
    const int status = ok ? (int)llrint(xa.frame[0]) : 0;
    rc[kRcStatus] = status;
    pub_store(&pub->rc_status, status);
    pub_store(&pub->rc_nf, m.counters[kCntFactors]);
    pub_flag(&pub->seq_rc, *seq_ctr);
  }
}
__global__ void __launch_bounds__(256) k_factor_finish_dev(const int* __restrict__ rc, DevMap m,
                                                           const int* __restrict__ fac_node,
                                                           double* __restrict__ fac_eig, Clu* __restrict__ fac_pcr) {
  if (rc[kRcStatus]) return;
  const int nf = m.counters[kCntFactors];
  for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < nf; a += gridDim.x * blockDim.x) {
    const int node = fac_node[a];
    m.hdr[node].opt_state = a;
    for (int j = 0; j < 12; j++) fac_eig[(size_t)a * 12 + j] = m.eig[(size_t)node * 12 + j];
    fac_pcr[a] = m.pcr_add[node];
  }
}
const int* map_rc_status(vg_ctx* ctx) { return ctx->wk.rc + kRcStatus; }
// the factor bookkeeping an asynchronous recut left to a k_ba_init that did not come
int map_factor_finish(vg_ctx* ctx) {
  if (!ctx->rc_finish_in_init) return VG_OK;
  ctx->rc_finish_in_init = false;
  k_factor_finish_dev<<<64, 256, 0, ctx->stream>>>(ctx->wk.rc, ctx->map, ctx->ba.fac_node, ctx->ba.fac_eig,
                                                   ctx->ba.fac_pcr);
  VG_HIP(hipGetLastError());
  return VG_OK;
}

// the host-sized rest of a recut whose device status (hrc) is in: insert
// replay request, level-overflow replay, factor sort and extraction
static int recut_complete(vg_ctx* ctx, const MP& mp, int nlev, int* hrc, int* n_factors) {
  Work& w = ctx->wk;
  hipStream_t s = ctx->stream;
  DevMap& m = ctx->map;
  WinD* dwin = (WinD*)ctx->ba.xs;
  auto list_of = [&](int L) { return (L % 2 == 1) ? w.list0 : w.list1; };
  if (hrc[kRcAbort] == kInsAbort) return kNeedInsertReplay;
  if (hrc[kRcAbort]) {  // replay from the level that overflowed on the host-sized path
    const int L0 = hrc[kRcAbort] - 1;
#ifdef VG_PROBE
    fprintf(stderr, "PROBE recut overflow replay from level %d (nsub=%d nwin=%d)\n", L0, hrc[kRcSub + L0],
            hrc[kRcWin + L0]);
#endif
    VG_HIP(hipMemsetAsync(w.rc + kRcAbort, 0, sizeof(int), s));
    VG_TRY(recut_slow_apply(ctx, L0, mp, dwin, list_of(L0 + 1), hrc));
    for (int L = L0 + 1; L < nlev; L++) {
      k_rc_visit<<<256 * kBlock / kSpreadBlock, kSpreadBlock, 0, s>>>(L, ctx->rc_thread_num, list_of(L), mp, m, list_of(L + 1), sub_of(w, L), w.cand,
                                        w.rc, nullptr);
      k_rc_win<<<256, 64 * kRcWinWaves, 0, s>>>(L, sub_of(w, L), dwin, m, ev_of(w, L), info_of(w, L), w.cap, w.cap, w.rc);
      VG_TRY(read_rc(ctx, hrc));
      VG_TRY(recut_slow_apply(ctx, L, mp, dwin, list_of(L + 1), hrc));
    }
  }
  VG_HIP(hipMemsetAsync(w.rc + kRcStatus, 0, sizeof(int), s));  // the LM rerun reads it
  VG_TRY(read_counters(ctx));
  const int nf = ctx->h_pinned[kCntFactors];
  if (nf > ctx->ba.cap_f) {
    ctx->err = "factor capacity exceeded";
    return VG_E_CAPACITY;
  }
  if (nf > 0) {
    int* sorted = w.cand;
    VG_TRY(sort_ids(ctx, w.cand, nf, &sorted));
    k_factor_finish<<<grid_for(nf), kBlock, 0, s>>>(nf, sorted, m, ctx->ba.fac_node, ctx->ba.fac_eig,
                                                    ctx->ba.fac_pcr);
    VG_HIP(hipGetLastError());
  }
  *n_factors = nf;
  return VG_OK;
}

__global__ void k_copy_int(const int* __restrict__ src, int* __restrict__ dst) {
  if (threadIdx.x == 0) *dst = *src;
}

// multi_recut (local_mapping.cpp:144-201) then tras_opt. Synchronous
// (pub_seq == 0): returns the factor count, or kNeedInsertReplay when the
// preceding insert must be replayed first (nothing of the recut ran).
// Asynchronous (pub_seq > 0): the factor extraction is sized on the device and
// nothing waits; *n_factors = -1 and the status arrives with Pub::seq_rc ==
// pub_seq (map_recut_resume completes a recut that needs the host).
static int map_recut_impl(vg_ctx* ctx, const MP& mp, const WinArg& wa, int thread_num, int* n_factors, bool replay,
                          int pub_seq) {
  DevMap& m = ctx->map;
  Work& w = ctx->wk;
  hipStream_t s = ctx->stream;
  *n_factors = 0;
  // the window view (poses from the device state, ring, per-ord counts)
  WinD* dwin = (WinD*)ctx->ba.xs;
  int* dn = (int*)((char*)ctx->ba.xs + sizeof(WinD));
  int* dslot = dn + 32;
  int total = 0;
  for (int i = 0; i < wa.win_count; i++) total += wa.nper[i];
  ctx->rc_total = total;
  ctx->rc_thread_num = thread_num;
  if (ctx->rc_begun) {  // done by the insert's k_push_window (the same graph)
    ctx->rc_begun = false;
  } else {
    k_make_win_recut_begin<<<1, 256, 0, s>>>(ctx->st, wa, ctx->map.wpn, dwin, dn, dslot, m, w.rc, thread_num);
  }
  if (sharded(ctx)) {
    if (!replay) {  // the global slide count (a replay re-uses it: the insert replay does not change it)
      VG_TRY(shard_allreduce(ctx, m.counters + kCntGSlide, ctx->shard.d_buf + 512, 1, 1, 2));
    }
    k_copy_int<<<1, 64, 0, s>>>((const int*)(ctx->shard.d_buf + 512), m.counters + kCntGSlide);
  }
  const int nlev = mp.max_layer + 1;  // children sit one layer down; leaves at max_layer do not subdivide
  auto list_of = [&](int L) { return (L % 2 == 1) ? w.list0 : w.list1; };  // worklist of level L >= 1
  constexpr int gv = 256;
  const int sub_cap = (ctx->dbg_apply_cap >= 0 && ctx->dbg_apply_cap < kApplySub) ? ctx->dbg_apply_cap : kApplySub;
  uint32_t* bits = pub_seq > 0 ? w.cand_bits : nullptr;
  if (ctx->rc_fused) {  // one launch per level boundary (k_rc_level0, k_rc_level)
    static_assert(gv <= kClkRcBlocks, "recut clock slots");
    k_rc_level0<<<gv, 64 * kRcFusedWaves, 0, s>>>(thread_num, mp, m, list_of(1), sub_of(w, 0), w.cand, w.rc, bits,
                                                 dwin, ev_of(w, 0), info_of(w, 0), w.cap, &ctx->st->clk,
                                                 mp.max_layer == 0 ? 1 : 0);
    for (int L = 0; L < mp.max_layer; L++)
      k_rc_level<<<gv, 64 * kRcFusedWaves, 0, s>>>(L, sub_cap, mp, m, sub_of(w, L), info_of(w, L), ev_of(w, L),
                                                  list_of(L + 1), list_of(L + 2), sub_of(w, L + 1), w.cand, w.rc,
                                                  bits, dwin, ev_of(w, L + 1), info_of(w, L + 1), w.cap, &ctx->st->clk,
                                                  L == mp.max_layer - 1 ? 1 : 0);
  } else {
    for (int L = 0; L < nlev; L++) {
      k_rc_visit<<<gv * kBlock / kSpreadBlock, kSpreadBlock, 0, s>>>(L, thread_num, L > 0 ? list_of(L) : nullptr, mp, m,
                                                                     list_of(L + 1), sub_of(w, L), w.cand, w.rc, bits);
      // nodes at layer max_layer never subdivide (recut_visit_node, octree.cpp:371-372):
      // the deepest level has no window events, no apply and no pushes
      if (L == mp.max_layer) break;
      k_rc_win<<<256, 64 * kRcWinWaves, 0, s>>>(L, sub_of(w, L), dwin, m, ev_of(w, L), info_of(w, L), w.cap, w.cap,
                                                w.rc);
      k_rc_apply<<<1, kApplyThreads, 0, s>>>(L, sub_cap, m, list_of(L + 1), sub_of(w, L), info_of(w, L),
                                             (int*)w.ac_off, w.rc);
      k_rc_push<<<64, 64 * kRcPushWaves, 0, s>>>(L, ev_of(w, L), (const int*)w.ac_off, mp, dwin, m, w.rc);
    }
  }
  VG_HIP(hipGetLastError());
  if (pub_seq > 0) {
    const int max_fac = (ctx->dbg_fac_max >= 0 && ctx->dbg_fac_max < kFacMax) ? ctx->dbg_fac_max : kFacMax;
    const bool shard_on = sharded(ctx);
    Shard& sh = ctx->shard;
    const XchgArg xa{shard_on ? sh.d_frame : nullptr, sh.d_seq, m.counters + kCntErr, kShardSmall, sh.world};
    k_fac_sort<<<1, 1024, 0, s>>>(m, w.rc, w.cand_bits, ctx->ba.fac_node, ctx->ba.cap_f, ctx->d_pub,
                                  &ctx->st->rc_ctr, max_fac, xa);
    if (shard_on) {
      VG_TRY(shard_exchange(ctx, kShardSmall));
      k_pub_rc<<<1, 64, 0, s>>>(m, w.rc, ctx->d_pub, &ctx->st->rc_ctr, xa);
    }
    if (ctx->rc_init_finish) {  // the LM's k_ba_init (next on the stream) does tras_opt's bookkeeping
      ctx->rc_finish_in_init = true;
    } else {
      k_factor_finish_dev<<<64, 256, 0, s>>>(w.rc, m, ctx->ba.fac_node, ctx->ba.fac_eig, ctx->ba.fac_pcr);
    }
    VG_HIP(hipGetLastError());
    *n_factors = -1;
    return VG_OK;
  }
  int* hrc = ctx->h_pinned + 128;
  VG_TRY(read_rc(ctx, hrc));
  return recut_complete(ctx, mp, nlev, hrc, n_factors);
}

// complete an asynchronous recut whose published status was nonzero (the LM
// skipped): same outcomes as the synchronous call
static int map_recut_resume_impl(vg_ctx* ctx, const MP& mp, int* n_factors) {
  int* hrc = ctx->h_pinned + 128;
  VG_TRY(read_rc(ctx, hrc));
  return recut_complete(ctx, mp, mp.max_layer + 1, hrc, n_factors);
}

// the recut's end on the main stream: the margi prefix (second stream) starts
// from it, under the LM iterations enqueued behind it
int map_recut(vg_ctx* ctx, const MP& mp, const WinArg& wa, int thread_num, int* n_factors, bool replay,
              int pub_seq) {
  const int r = map_recut_impl(ctx, mp, wa, thread_num, n_factors, replay, pub_seq);
  if (!ctx->capturing) VG_HIP(hipEventRecord(ctx->ev_recut_done, ctx->stream));  // else after the graph launch
  return r;
}
int map_recut_resume(vg_ctx* ctx, const MP& mp, int* n_factors) {
  const int r = map_recut_resume_impl(ctx, mp, n_factors);
  VG_HIP(hipEventRecord(ctx->ev_recut_done, ctx->stream));
  return r;
}

}  // namespace vg

#ifdef VG_PROBE
VG_PROBE_READER(vg_probe_read_recut)
#endif
