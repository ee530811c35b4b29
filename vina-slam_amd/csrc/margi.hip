// margi.hip — marginalisation of the device-resident voxel map (map.hip).
//
// SURVEY §8(a) rows:
//   A10 multi_margi -> OctoTree::margi    local_mapping.cpp:17-84, octree.cpp:302-333, 395-495
#include "vg_map.h"

namespace vg {

// ------------------------------------------------------------------ margi (A10)
// collect every node under the slide roots, level by level (top-down)
// level L of the surf_map_slide subtrees: level 0 is m.slide itself, levels
// >= 1 sit back to back in `lists` (level L at the sum of the counts of levels
// 1..L-1; the count of level L+1 is rc[L], appended by level L)
__device__ __forceinline__ int margi_level(int L, const DevMap& m, const int* rc, int* lists, int** work) {
  if (L == 0) {
    *work = m.slide;
    return m.counters[kCntSlide];
  }
  int off = 0;
  for (int l = 1; l < L; l++) off += rc[l - 1];
  *work = lists + off;
  return rc[L - 1];
}

// OctoTree::margi's bottom-up isexist (octree.cpp:485-494) without a launch
// per level: a node whose isexist is final reports it to its parent with one
// 64-bit atomic (children still to report in the high word, minus one; the
// existing ones in the low word, plus its bit); the child that reports last
// has every sibling's bit in the returned word, so it sets the parent's
// isexist = OR(children) and reports for the parent in turn. The payload is
// the atomic itself: no fence. Roots (parent -1) end the chain.
__device__ __forceinline__ void margi_exist_up(DevMap& m, int node, int ex) {
  for (int hop = 0; hop < 16; hop++) {
    const int par = m.hdr[node].parent;
    if (par < 0) return;
    const unsigned long long old = atomicAdd(&m.pend[par], (unsigned long long)ex - (1ull << 32));
    if ((old >> 32) != 1ull) return;  // a sibling reports later
    ex = ((unsigned)(old & 0xffffffffull) + (unsigned)ex) > 0u ? 1 : 0;
    m.hdr[par].isexist = (int8_t)ex;
    node = par;
  }
}

__global__ void __launch_bounds__(256) k_collect_level(int L, int thread_num, DevMap m, int* __restrict__ lists,
                                                       int* __restrict__ leaves, int* __restrict__ rc) {
  if (g_slide(m) < thread_num) return;
  int* work;
  const int nw = margi_level(L, m, rc, lists, &work);
  int* next;
  (void)margi_level(L + 1, m, rc, lists, &next);  // its count is still being appended
  const int next_off = (int)(next - lists);
  for (int base = blockIdx.x * blockDim.x; base < nw; base += gridDim.x * blockDim.x) {
    const int q = base + threadIdx.x;
    const int node = q < nw ? work[q] : -1;
    int nchild = 0, is_leaf = 0;
    int kids[8];
    if (node >= 0) {
      NodeHdr& h = m.hdr[node];
      if (h.octo == 1) {
        for (int o = 0; o < 8; o++)
          if (h.child[o] >= 0) kids[nchild++] = h.child[o];
        m.pend[node] = (unsigned long long)nchild << 32;  // margi_exist_up: children still to report
        if (nchild == 0) {  // internal_exist of a childless node: 0, reported now
          h.isexist = 0;
          margi_exist_up(m, node, 0);
        }
      } else {
        is_leaf = 1;
      }
    }
    int o1 = wave_append(&rc[L], nchild);
    int o2 = wave_append(&m.counters[kCntLeaves], is_leaf);
    if (next_off + o1 + nchild > m.cap_nodes) {
      atomicOr(&m.counters[kCntErr], 4);
      continue;
    }
    for (int j = 0; j < nchild; j++) next[o1 + j] = kids[j];
    if (is_leaf) leaves[o2] = node;
  }
}

__device__ void plane_update_dev(DevMap& m, int node, const Clu& pcr_add, const double* e) {
  PlaneRec& P = m.pl[node];
  V3 center = v3(pcr_add.v[0] / pcr_add.N, pcr_add.v[1] / pcr_add.N, pcr_add.v[2] / pcr_add.N);
  V3 u[3];
  for (int k = 0; k < 3; k++) u[k] = v3(e[3 + 0 * 3 + k], e[3 + 1 * 3 + k], e[3 + 2 * 3 + k]);
  double nv = 1.0 / pcr_add.N;
  M<3, 9> uc;
  uc.zero();
  const int l = 0;
  for (int k = 1; k < 3; k++) {
    M3 ukl = outer3(u[k], u[l]);
    double f[9];
    f[0] = ukl(0, 0);
    f[1] = ukl(1, 0) + ukl(0, 1);
    f[2] = ukl(2, 0) + ukl(0, 2);
    f[3] = ukl(1, 1);
    f[4] = ukl(1, 2) + ukl(2, 1);
    f[5] = ukl(2, 2);
    double a1 = dot3(u[k], center), a2 = dot3(u[l], center);
    for (int j = 0; j < 3; j++) f[6 + j] = -(u[l][j] * a1 + u[k][j] * a2);
    double sc = nv / (e[l] - e[k]);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 9; c++) uc(r, c) += (u[k][r] * sc) * f[c];
  }
  M<9, 9> cov = unpack9(&m.cov_add[(size_t)node * kCovN]);
  M<3, 9> Jc = mul(uc, cov);
  M3 A = mul(Jc, tr(uc));
  double pv[6][6];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      pv[r][c] = A(r, c);
      pv[r][3 + c] = Jc(r, 6 + c) * nv;
      pv[3 + c][r] = pv[r][3 + c];
      pv[3 + r][3 + c] = cov(6 + r, 6 + c) * (nv * nv);
    }
  for (int r = 0; r < 6; r++)
    for (int c = r; c < 6; c++) P.var[sym_idx(6, r, c)] = pv[r][c];
  for (int j = 0; j < 3; j++) {
    P.center[j] = center[j];
    P.normal[j] = u[0][j];
  }
  P.radius = (float)e[2];
}

// OctoTree::margi leaf branch (octree.cpp:397-484), mgsize = 1. A leaf's
// run of the oldest slot (DevMap::lseg) is its sw->points[mp[0]] list in push
// order.
__global__ void __launch_bounds__(256) k_margi_leaf(const int* __restrict__ nleaves, const int* __restrict__ leaves,
                                                    MP mp, WinArg wa, DState* __restrict__ st, WinD* __restrict__ win,
                                                    int* __restrict__ nper, int* __restrict__ slot_of, int ba_iters_valid,
                                                    const int* __restrict__ ba_iters, const int* __restrict__ ba_hess,
                                                    Pub* __restrict__ pub, int seq, DevMap m,
                                                    const double* __restrict__ fac_eig, const Clu* __restrict__ fac_pcr,
                                                    int* __restrict__ plan, const int* __restrict__ gate,
                                                    unsigned* __restrict__ head_flag, int batch,
                                                    const int* __restrict__ dseq, const unsigned* __restrict__ pre_flag,
                                                    int mk_on) {
  if (gate && !*gate) return;  // a speculative tail the LM did not reach (ba_run)
  if (pre_flag && blockIdx.x > 0) {  // the scan graph: the leaves read the margi prefix's lists (d_sync[4] >= ph[4])
    // Normally the prefix ended long before (it runs under the LM): its
    // writes were released at its end and this kernel's start acquired them,
    // so no fence. Only a workgroup that had to wait acquires after the wait
    // (an agent-scope acquire per workgroup invalidates the XCD's L2: with
    // ~2k workgroups that cost the kernel 14 us when every one did it)
    __shared__ int s_state;  // 0 ready at once, 1 waited, 2 timed out
    if (threadIdx.x == 0) {
      const unsigned t = (unsigned)st->ph[4];
      int state = 0;
      for (long it = 0; (int)(__hip_atomic_load(pre_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - t) < 0; it++) {
        state = 1;
        __builtin_amdgcn_s_sleep(4);
        if (it > (1l << 24)) {
          state = 2;
          atomicOr(&m.counters[kCntErr], 64);
          break;
        }
      }
      s_state = state;
    }
    __syncthreads();
    if (s_state == 2) return;
    if (s_state == 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  if (blockIdx.x == 0) {  // the margi head: x_curr <- x_buf.back(), the window view, the state publication
    if (dseq) {  // the scan graph: this scan's publication numbers from the device state (DState::ph)
      seq = dseq[0];
      wa.seq2 = dseq[1];
      wa.jour_check = dseq[4];
    }
    make_win_block(st, wa, m.wpn, win, nper, slot_of);
    __syncthreads();  // x_curr (set_xc), seen by the whole block
    if (threadIdx.x == 0) st->margi_seq = seq;  // k_margi_copy hands it to the next IEKF
    // x_curr is final: the next scan's propagation may start (vg_ctx::d_sync[2]) as soon as
    // the publication has read what that propagation overwrites
    publish_state_block(st, wa.win_count, ba_iters_valid, ba_iters, ba_hess, pub, seq, head_flag, (unsigned)seq);
    return;
  }
  // the leaves read the refined window poses from the state (the view block
  // above writes the same values into *win for the later margi kernels)
  const double* xs = st->xs;
  const int nl = *nleaves;
#ifdef VG_PROBE
  const unsigned long long pt0 = wall_clock64();
  const bool pwork = (int)((blockIdx.x - 1) * blockDim.x) < nl;
#endif
  int n_pu = 0, n_full = 0;  // plane_update calls / leaves past max_points (per-scan counters)
#ifdef VG_PROBE
  // per leaf thread, summed over the live leaves (scripts/probe_margi.py): 51 header + run + own
  // cluster, 52 frame clusters + merge + eigen, 54 plane update, 55 point_fix carve + stores;
  // 56 live leaves, 57 the longest leaf, 58 factor leaves
  unsigned long long pq0 = wall_clock64(), pa = 0, pb2 = 0, pc = 0, pd = 0, ptot = 0, nlive = 0, nfac = 0;
#define PMG(v)                                   \
  do {                                           \
    const unsigned long long n_ = wall_clock64(); \
    v += n_ - pq0;                               \
    pq0 = n_;                                    \
  } while (0)
#else
#define PMG(v) (void)0
#endif
  // whole waves per round: the point_fix blocks that grow are carved with one
  // atomic per wave (wave_append) instead of one per leaf on the shared counter
  for (int base = (blockIdx.x - 1) * blockDim.x; base < nl; base += (gridDim.x - 1) * blockDim.x) {
    const int q = base + threadIdx.x;
    const int node = q < nl ? leaves[q] : -1;
    int* pq = &plan[(size_t)(q < nl ? q : 0) * 8];
    if (node >= 0) {
      pq[0] = -1;  // no point_fix copies (k_margi_copy)
      pq[4] = 0;
    }
    const bool live = node >= 0 && m.hdr[node].isexist && m.hdr[node].has_sw;
    const int W = mp.W;
    const int s0 = wa.mp[0];
#ifdef VG_PROBE
    const unsigned long long pstart = wall_clock64();
    pq0 = pstart;
#endif
    int seg = -1, segn = 0;  // the leaf's run of the oldest slot: its sw->points[mp[0]] in push order
    Clu w0, add_, fix_;
    int grow = 0;  // size of a new point_fix block (the live one is full)
    bool append = false;
    if (live) {
      NodeHdr& h = m.hdr[node];
      if (!lseg_get(m, node, s0, seg, segn)) seg = -1;
      Clu* loc = &m.pcrs[(size_t)node * W];
      const M3 R0 = ld_m3(xs);
      const V3 p0 = ld_v3(xs + 9);
      clu_zero(w0);
      if (loc[s0].N != 0) w0 = clu_transform(loc[s0], R0, p0);
      double* e = &m.eig[(size_t)node * 12];
      PMG(pa);
#ifdef VG_PROBE
      if (h.opt_state >= 0) nfac++;
#endif
      if (h.opt_state >= 0) {
        add_ = fac_pcr[h.opt_state];
        for (int j = 0; j < 12; j++) e[j] = fac_eig[(size_t)h.opt_state * 12 + j];
        h.opt_state = -1;
      } else {
        add_ = m.pcr_fix[node];
        if (batch) {  // the frame clusters read four at a time (one round trip each four), merged in frame order
          for (int i0 = 0; i0 < wa.win_count; i0 += 4) {
            Clu c[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
              if (i0 + k < wa.win_count) c[k] = loc[wa.mp[i0 + k]];
#pragma unroll
            for (int k = 0; k < 4; k++) {
              const int i = i0 + k;
              if (i < wa.win_count && c[k].N != 0) {
                Clu t = (i == 0) ? w0 : clu_transform(c[k], ld_m3(xs + (size_t)i * kXS), ld_v3(xs + (size_t)i * kXS + 9));
                clu_add(add_, t);
              }
            }
          }
        } else {
          for (int i = 0; i < wa.win_count; i++) {
            int si = wa.mp[i];
            if (loc[si].N != 0) {
              Clu t = (i == 0) ? w0 : clu_transform(loc[si], ld_m3(xs + (size_t)i * kXS), ld_v3(xs + (size_t)i * kXS + 9));
              clu_add(add_, t);
            }
          }
        }
        if (h.is_plane) {
          V3 ev;
          M3 U;
          eig3(clu_cov(add_), ev, U);
          for (int j = 0; j < 3; j++) e[j] = ev[j];
          for (int j = 0; j < 9; j++) e[3 + j] = U[j];
        }
      }
      fix_ = m.pcr_fix[node];
      PMG(pb2);
      if (fix_.N < mp.max_points && h.is_plane)
        if (add_.N - h.last_num >= 5 || h.last_num <= 10) {
          plane_update_dev(m, node, add_, e);
          h.last_num = add_.N;
          if (mk_on) h.mk |= kMkUpdated;  // plane.is_update / is_normal_update (octree.cpp:441-446), markers.hip
          n_pu++;
        }
      PMG(pc);
      if (fix_.N >= mp.max_points) n_full++;
      if (fix_.N < mp.max_points) {
        if (w0.N != 0) {
          clu_add(fix_, w0);
          if (seg >= 0 && segn > 0) {
            append = true;
            const int need = h.fix_cnt + segn;
            if (need > h.fix_cap) grow = need * 2 < 128 ? 128 : need * 2;
          }
        }
      } else {
        if (w0.N != 0) clu_sub(add_, w0);
        h.fix_cnt = 0;
      }
    }
    const int off = wave_append(&m.counters[kCntFix], grow);
    if (live) {
      NodeHdr& h = m.hdr[node];
      bool ok = true;
      if (append) {
        if (grow > 0) {  // grow the point_fix block (old block is abandoned)
          if (off + grow > m.cap_fix) {
            atomicOr(&m.counters[kCntErr], 8);
            ok = false;
          } else {
            pq[0] = h.fix_off;  // grow: move the live block first
            pq[1] = h.fix_cnt;
            pq[2] = off;
            h.fix_off = off;
            h.fix_cap = grow;
          }
        }
        if (ok) {
          pq[3] = seg;  // then append the oldest frame's points of this leaf
          pq[4] = segn;
          pq[5] = h.fix_off + h.fix_cnt;
          h.fix_cnt += segn;
        }
      }
      if (ok) {
        clu_zero(m.pcrs[(size_t)node * W + s0]);
        m.pcr_fix[node] = fix_;
        m.pcr_add[node] = add_;
        h.isexist = (fix_.N >= add_.N) ? 0 : 1;
      }
#ifdef VG_PROBE
      PMG(pd);
      const unsigned long long tl = wall_clock64() - pstart;
      ptot = tl > ptot ? tl : ptot;
      nlive++;
#endif
    }
  }
#undef PMG
#ifdef VG_PROBE
  {
    unsigned long long v[7] = {pa, pb2, pc, pd, nlive, nfac, ptot};
    for (int off = 32; off > 0; off >>= 1)
      for (int k = 0; k < 7; k++) {
        const unsigned long long o = __shfl_xor(v[k], off, 64);
        v[k] = k == 6 ? (o > v[k] ? o : v[k]) : v[k] + o;
      }
    if ((threadIdx.x & 63) == 0 && blockIdx.x > 0 && v[4] > 0) {  // working waves only (few atomics)
      atomicAdd(&g_probe[51], v[0]);
      atomicAdd(&g_probe[52], v[1]);
      atomicAdd(&g_probe[54], v[2]);
      atomicAdd(&g_probe[55], v[3]);
      atomicAdd(&g_probe[56], v[4]);
      atomicAdd(&g_probe[58], v[5]);
      atomicMax(&g_probe[57], v[6]);
    }
  }
#endif
  wave_append(&m.counters[kCntPlaneUpd], n_pu);
  wave_append(&m.counters[kCntFixFull], n_full);
#ifdef VG_PROBE
  __syncthreads();
  if (threadIdx.x == 0 && pwork) {  // per working block: summed span, longest span, count; leaves
    const unsigned long long pt1 = wall_clock64();
    atomicAdd(&g_probe[46], pt1 - pt0);
    atomicMax(&g_probe[45], pt1 - pt0);
    atomicAdd(&g_probe[47], 1ull);
    atomicMax(&g_probe[50], (unsigned long long)nl);
  }
#endif
}

// the point_fix copies planned by k_margi_leaf, one wave per leaf: the live
// block moves when it grows, then the leaf's points of the oldest frame are
// appended in push order (octree.cpp:450-458)
constexpr int kCopyWaves = 4;
// exist_up: the leaves also report their isexist up the tree (margi_exist_up,
// k_margi_erase_all follows); each leaf's report rides on a lane of its own
__global__ void __launch_bounds__(64 * kCopyWaves) k_margi_copy(const int* __restrict__ nleaves,
                                                                const int* __restrict__ plan,
                                                                const WinD* __restrict__ win, DevMap m, const int* __restrict__ gate,
                                                                const int* __restrict__ leaves, int exist_up,
                                                                unsigned* __restrict__ tail_flag,
                                                                const DState* __restrict__ st) {
  if (gate && !*gate) return;  // a speculative tail the LM did not reach (ba_run)
  // k_margi_leaf (the plane updates the next IEKF reads) has ended: its writes
  // are released, so the hand-off flag to the IEKF stream goes up now, with
  // the margi head's number (no k_sync_set launch between the two kernels)
  if (tail_flag && blockIdx.x == 0 && threadIdx.x == 0)
    __hip_atomic_store(tail_flag, (unsigned)st->margi_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int lane = threadIdx.x & 63;
  const int nl = *nleaves;
  if (exist_up)
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nl; q += gridDim.x * blockDim.x) {
      const int node = leaves[q];
      margi_exist_up(m, node, m.hdr[node].isexist ? 1 : 0);
    }
  const int s0 = win->mp[0];
  const M3 R0 = ld_m3(win->R[0]);
  const V3 p0 = ld_v3(win->p[0]);
  for (int q = blockIdx.x * kCopyWaves + (threadIdx.x >> 6); q < nl; q += gridDim.x * kCopyWaves) {
    const int* pq = &plan[(size_t)q * 8];
    const int src = pq[0], segn = pq[4];
    if (src >= 0) {
      const int nold = pq[1], dst = pq[2];
      for (int j = lane; j < nold; j += 64) {
        const size_t a = (size_t)src + j, b = (size_t)dst + j;
        for (int t = 0; t < 3; t++) m.fix_pnt[b * 3 + t] = m.fix_pnt[a * 3 + t];
        for (int t = 0; t < 9; t++) m.fix_var[b * 9 + t] = m.fix_var[a * 9 + t];
      }
    }
    if (segn > 0) {
      const int seg = pq[3], dst = pq[5];
      for (int j = lane; j < segn; j += 64) {
        const int i = m.wp_ord[(size_t)s0 * m.ord_stride + seg + j];
        const size_t b = (size_t)s0 * m.cap_wp + i;
        const V3 pt = rigid(R0, ld_v3(&m.wp_pnt[b * 3]), p0);
        const size_t d = (size_t)dst + j;
        for (int t = 0; t < 3; t++) m.fix_pnt[d * 3 + t] = pt[t];
        for (int t = 0; t < 9; t++) m.fix_var[d * 9 + t] = m.wp_var[b * 9 + t];
      }
    }
  }
}

// internal nodes bottom-up: isexist = OR(children) (octree.cpp:485-494); the
// deepest level's launch also clears the oldest-slot segment records
__device__ __forceinline__ void internal_exist(DevMap& m, int node) {
  NodeHdr& h = m.hdr[node];
  if (h.octo != 1) return;
  int8_t e = 0;
  for (int o = 0; o < 8; o++)
    if (h.child[o] >= 0) e |= m.hdr[h.child[o]].isexist;
  h.isexist = e ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_margi_internal(int L, int thread_num, DevMap m, int* __restrict__ lists,
                                                        const int* __restrict__ rc, const int* __restrict__ gate) {
  if (gate && !*gate) return;  // a speculative tail the LM did not reach (ba_run)
  if (g_slide(m) < thread_num) return;
  int* work;
  const int nw = margi_level(L, m, rc, lists, &work);
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nw; q += gridDim.x * blockDim.x) internal_exist(m, work[q]);
}

// erase dead roots from surf_map_slide (local_mapping.cpp:67-78) with
// clear_slwd over their subtrees (octree.cpp:739-756), top-down. Level 0 also
// finishes the bottom-up isexist pass (its roots are level 0's own nodes);
// level L also resets the dead marks of level L-2, which nobody reads any more.
__global__ void __launch_bounds__(256) k_margi_erase_mark(int L, int thread_num, DevMap m, int* __restrict__ lists,
                                                          const int* __restrict__ rc, const int* __restrict__ gate) {
  if (gate && !*gate) return;  // a speculative tail the LM did not reach (ba_run)
  if (g_slide(m) < thread_num) return;
  int* work;
  const int nw = margi_level(L, m, rc, lists, &work);
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nw; q += gridDim.x * blockDim.x) {
    int node = work[q];
    NodeHdr& h = m.hdr[node];
    int dead;
    if (L == 0) {
      internal_exist(m, node);
      dead = h.isexist ? 0 : 1;
    } else {
      dead = m.nscr[(size_t)h.parent * 4 + 2] == 7 ? 1 : 0;
    }
    if (dead) {
      m.nscr[(size_t)node * 4 + 2] = 7;
      h.has_sw = 0;
      for (int j = 0; j < m.W; j++) clu_zero(m.pcrs[(size_t)node * m.W + j]);
      if (L == 0) m.in_slide[node] = 0;
    }
  }
  if (L >= 2) {
    const int nc = margi_level(L - 2, m, rc, lists, &work);
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nc; q += gridDim.x * blockDim.x)
      m.nscr[(size_t)work[q] * 4 + 2] = -1;
  }
}
// reset the dead marks of levels L0 .. nlev-1
__global__ void __launch_bounds__(256) k_clear_mark(int L0, int nlev, int thread_num, DevMap m,
                                                    int* __restrict__ lists, const int* __restrict__ rc, const int* __restrict__ gate) {
  if (gate && !*gate) return;  // a speculative tail the LM did not reach (ba_run)
  if (g_slide(m) < thread_num) return;
  for (int L = L0 < 0 ? 0 : L0; L < nlev; L++) {
    int* work;
    const int nw = margi_level(L, m, rc, lists, &work);
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nw; q += gridDim.x * blockDim.x)
      m.nscr[(size_t)work[q] * 4 + 2] = -1;
  }
}
// local_mapping.cpp:67-78 + clear_slwd (octree.cpp:739-756) in one launch: a
// node of the slide subtrees is erased with its root, so every node of every
// level looks its root up (L parent hops) — the roots' isexist is final
// (margi_exist_up) — instead of a top-down launch per level with dead marks
__global__ void __launch_bounds__(256) k_margi_erase_all(int nlev, int thread_num, DevMap m, const int* __restrict__ lists,
                                                         const int* __restrict__ rc, const int* __restrict__ gate) {
  if (gate && !*gate) return;  // a speculative tail the LM did not reach (ba_run)
  if (g_slide(m) < thread_num) return;
  const int n0 = m.counters[kCntSlide];
  int total = n0;
  for (int l = 1; l < nlev; l++) total += rc[l - 1];
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < total; q += gridDim.x * blockDim.x) {
    int L = 0, node;
    if (q < n0) {
      node = m.slide[q];
    } else {
      int r = q - n0, off = 0;
      L = 1;
      while (L < nlev - 1 && r >= rc[L - 1]) {
        r -= rc[L - 1];
        off += rc[L - 1];
        L++;
      }
      node = lists[off + r];
    }
    int root = node;
    for (int k = 0; k < L; k++) root = m.hdr[root].parent;
    if (!m.hdr[root].isexist) {
      m.hdr[node].has_sw = 0;
      for (int j = 0; j < m.W; j++) clu_zero(m.pcrs[(size_t)node * m.W + j]);
      if (L == 0) m.in_slide[node] = 0;
    }
  }
}

// single block, order-preserving in-place compaction of the slide list (a
// chunk is read completely before any of it is written; writes never pass
// the read position)
// then (the same workgroup) the x_buf / imu_pre_buf slide of the device state
// (local_mapping.cpp:536-546) and the end-of-scan counter publication
__global__ void __launch_bounds__(1024) k_slide_compact(int thread_num, DevMap m, DState* __restrict__ st, int wc,
                                                        int nimu, Pub* __restrict__ pub, int seq2, const int* __restrict__ gate) {
  if (gate && !*gate) return;  // a speculative tail the LM did not reach (ba_run)
  if (threadIdx.x == 0 && st->jour_check && wc > 0) {  // local_mapping.cpp:510-518, x_curr.p = x_buf.back().p
    const double* xb = st->xs + (size_t)(wc - 1) * kXS + 9;  // (read before the slide below)
    const V3 p = v3(xb[0], xb[1], xb[2]);
    const double spat = norm3(sub(p, v3(st->last_pos[0], st->last_pos[1], st->last_pos[2])));
    if (spat > 0.5) {
      st->jour += spat;
      for (int j = 0; j < 3; j++) st->last_pos[j] = p[j];
    }
    st->jour_check = 0;
  }
  __shared__ int base;
  __shared__ int sc[1024];
  __shared__ int s_w[17];
  const int n = m.counters[kCntSlide];
  constexpr int kPer = 16;
  if (g_slide(m) >= thread_num && n <= kPer * (int)blockDim.x) {
    // one pass: every lane reads a contiguous run into registers, one block
    // scan orders the survivors (all reads precede the scan's barriers, so the
    // in-place writes cannot overtake them)
    const int per = (n + (int)blockDim.x - 1) / (int)blockDim.x;
    const int q0 = threadIdx.x * per;
    int nodes[kPer];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
      const int q = q0 + k;
      int node = (k < per && q < n) ? m.slide[q] : -1;
      if (node >= 0 && !m.in_slide[node]) node = -1;
      nodes[k] = node;
      cnt += node >= 0 ? 1 : 0;
    }
    int total;
    int pos = block_excl_scan(cnt, s_w, &total);
#pragma unroll
    for (int k = 0; k < kPer; k++)
      if (nodes[k] >= 0) m.slide[pos++] = nodes[k];
    if (threadIdx.x == 0) m.counters[kCntSlide] = total;
  } else if (g_slide(m) >= thread_num) {
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int start = 0; start < n; start += blockDim.x) {
      const int q = start + threadIdx.x;
      const int node = q < n ? m.slide[q] : -1;
      const int keep = (node >= 0 && m.in_slide[node]) ? 1 : 0;
      sc[threadIdx.x] = keep;
      __syncthreads();
      for (int off = 1; off < (int)blockDim.x; off <<= 1) {
        int v = threadIdx.x >= (unsigned)off ? sc[threadIdx.x - off] : 0;
        __syncthreads();
        sc[threadIdx.x] += v;
        __syncthreads();
      }
      if (keep) m.slide[base + sc[threadIdx.x] - 1] = node;
      __syncthreads();
      if (threadIdx.x == blockDim.x - 1) base += sc[threadIdx.x];
      __syncthreads();
    }
    if (threadIdx.x == 0) m.counters[kCntSlide] = base;
  }
  const int t = threadIdx.x;
  const double v = (t < (wc - 1) * kXS) ? st->xs[kXS + t] : 0.0;
  const double b = (t < (nimu - 1) * 12) ? st->bias[12 + t] : 0.0;
  __syncthreads();
  if (t < (wc - 1) * kXS) st->xs[t] = v;
  if (t < (nimu - 1) * 12) st->bias[t] = b;
  if (t == 0) st->imu_head = (st->imu_head + 1) % kMaxWin;  // imu_pre_buf.pop_front (the record ring)
  if (seq2 < 0) seq2 = st->seq2;  // set by k_make_win (replayed graph)
  if (seq2 > 0) {
    __syncthreads();
    if (t < kCntN) pub_store(&pub->counters[t], m.counters[t]);
    pub_drain();
    __syncthreads();
    if (t == 0) pub_flag(&pub->seq2, seq2);
  }
}
__global__ void __launch_bounds__(256) k_set_jour(int thread_num, DevMap m, const double* __restrict__ jour,
                                                  int* __restrict__ rc, int n_oldest) {
  if (blockIdx.x == 0) {  // margi level counts and the leaf count start at zero
    // kRcStatus is the recut's (k_ba_init may read it concurrently on the main stream)
    for (int i = threadIdx.x; i < kRcN; i += blockDim.x)
      if (i != kRcStatus) rc[i] = (i == kRcNOld) ? n_oldest : 0;
    if (threadIdx.x == 0) m.counters[kCntLeaves] = 0;
  }
  const int n = m.counters[kCntSlide];
  if (g_slide(m) < thread_num) return;
  const double j = *jour;  // the device's jour (DState::jour, the previous margi's update)
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) m.jour[m.slide[q]] = j;
}

// multi_margi (local_mapping.cpp:21-78): every count stays on the device;
// the host enqueues max_layer+1 levels (no level can be deeper) and
// synchronises once at the end for the error flags.
// The part of multi_margi that does not depend on the BA (jour stamps, the
// slide-tree levels, the oldest slot's points grouped by leaf), enqueued right
// after the recut on the second stream so it runs under the LM iterations.
int map_margi_prefix(vg_ctx* ctx, const MP& mp, int slot0, int n_oldest, int thread_num, const unsigned* flags) {
  DevMap& m = ctx->map;
  Work& w = ctx->wk;
  hipStream_t s = ctx->stream_ds;
  const int nlev = mp.max_layer + 1;
  if (flags) {  // the scan graph: k_ba_init raises d_sync[3] once the recut has ended (no event inside a graph)
    VG_TRY(sync_wait(ctx, s, 3, flags[0]));
  } else {
    VG_HIP(flush_insert_events(ctx));
    VG_HIP(hipStreamWaitEvent(s, ctx->ev_recut_done, 0));  // recorded at the recut's end (map_recut)
  }
  const int gl = 64;  // grid-stride over device-side counts
  k_set_jour<<<gl, kBlock, 0, s>>>(thread_num, m, &ctx->st->jour, w.rc, n_oldest);
  for (int L = 0; L < nlev; L++) k_collect_level<<<gl * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(L, thread_num, m, w.list1, w.list0, w.rc);
  (void)slot0;  // the oldest slot's points per leaf are the leaves' runs (DevMap::lseg): no sort here
  (void)n_oldest;
  VG_HIP(hipGetLastError());
  if (flags) VG_TRY(sync_set(ctx, s, 4, flags[1]));  // the scan graph's margi tail waits for it
  VG_HIP(hipEventRecord(ctx->ev_prefix_done, s));
  return VG_OK;
}

// pub_localmap's /map_cmap cloud (publishers.cpp:102-119): every third point
// of the oldest window frame (mgsize = 1: pvec_buf[0]) at x_buf[0] after the
// BA, R pnt + p in fp64, stored as float like the PointType it publishes
__global__ void __launch_bounds__(256) k_local_map(const WinD* __restrict__ win, DevMap m, float4* __restrict__ out,
                                                   int* __restrict__ nout, const int* __restrict__ gate) {
  if (gate && !*gate) return;  // a speculative tail the LM did not reach (ba_run)
  const int slot = win->mp[0];
  const int n = m.wpn[slot];
  const int nk = (n + 2) / 3;
  if (blockIdx.x == 0 && threadIdx.x == 0) nout[0] = nk;
  const M3 R = ld_m3(win->R[0]);
  const V3 p = ld_v3(win->p[0]);
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nk; k += gridDim.x * blockDim.x) {
    const size_t b = (size_t)slot * m.cap_wp + 3 * k;
    const V3 w = rigid(R, ld_v3(&m.wp_pnt[b * 3]), p);
    out[k] = make_float4((float)w[0], (float)w[1], (float)w[2], m.wp_int[b]);
  }
}

int map_margi(vg_ctx* ctx, const MP& mp, const WinArg& wa, int n_oldest, int thread_num, int pub_seq,
              int pub_seq2, const int* gate) {
  DevMap& m = ctx->map;
  Work& w = ctx->wk;
  hipStream_t s = ctx->stream;
  const int nlev = mp.max_layer + 1;
  WinD* dwin = (WinD*)ctx->ba.xs;
  int* dn = (int*)((char*)ctx->ba.xs + sizeof(WinD));
  if (wa.win_count * kXS > 1024) {
    ctx->err = "win_size too large for the state slide";
    return VG_E_ARG;
  }
  // x_curr.R/p <- x_buf.back() and the window view (which also stores the
  // end-of-scan publication number); the state is then final for this scan
  // and is published — all by k_margi_leaf's workgroup 0, beside the leaves
  WinArg wa2 = wa;
  wa2.seq2 = pub_seq2;
  VG_HIP(hipStreamWaitEvent(s, ctx->ev_prefix_done, 0));  // map_margi_prefix
  // the rest reads every per-scan value from the device (n_oldest: rc, the
  // publication number: the state), so it is captured once and replayed
  const int gl = 64;
  // k_margi_leaf's plane updates are the last margi work the next scan's
  // IEKF reads: ev_tail_a marks them, and the remainder (point_fix copies,
  // isexist / erase marks, slide compaction, the device-state slide, the
  // counter publication; nothing the IEKF reads) runs under the next IEKF
  // one lane per leaf (eigen-decomposition + plane_update in series on the lane):
  // enough blocks that no lane takes two leaves, surplus blocks exit at once
  // workgroup 0 is the margi head (the window view and the state publication,
  // k_make_win_publish's work) running beside the leaves
  const int* bi = pub_seq > 0 ? ba_iters_dev(ctx) : nullptr;
  // the hand-off flags to the next scan's IEKF stream: the margi head's
  // x_curr (d_sync[2], the device propagation starts from it) and the leaves'
  // plane updates (d_sync[0], the IEKF reads them)
  // (sharded as well: the hand-offs are device-side only, and no exchange sits
  // between a flag's producer and its consumer)
  const bool flags = ctx->flag_sync && ctx->overlap_iekf && ctx->use_graphs && !ctx->prof_stages;
  k_margi_leaf<<<1 + 512 * kBlock / kSpreadBlock, kSpreadBlock, 0, s>>>(
      m.counters + kCntLeaves, w.list0, mp, wa2, ctx->st, dwin, dn, dn + 32, bi != nullptr, bi,
      bi ? ba_hess_dev(ctx) : nullptr, ctx->d_pub, pub_seq, m, ctx->ba.fac_eig, ctx->ba.fac_pcr, w.plan, gate,
      flags ? ctx->d_sync + 2 : nullptr, ctx->margi_batch ? 1 : 0, nullptr, nullptr, (ctx->pub_flags & 2) ? 1 : 0);
  VG_HIP(hipEventRecord(ctx->ev_tail_a, s));
  // the margi's publication number into the IEKF hand-off flag: by the margi
  // graph's first kernel (k_margi_copy) — or k_sync_set when the local map
  // publication sits in between
  const bool copy_signals = flags && !(ctx->pub_flags & 1);
  if (flags && !copy_signals) VG_TRY(sync_set(ctx, s, 0, (unsigned)pub_seq, gate));
  if (ctx->pub_flags & 1) k_local_map<<<64, kBlock, 0, s>>>(dwin, m, ctx->d_cmap, ctx->d_cmap_n, gate);
  ctx->tail_a_valid = true;
  auto body = [&]() -> int {
    const bool fused = ctx->margi_fused;
    k_margi_copy<<<256, 64 * kCopyWaves, 0, s>>>(m.counters + kCntLeaves, w.plan, dwin, m, gate, w.list0, fused ? 1 : 0,
                                                  copy_signals ? ctx->d_sync : nullptr, ctx->st);
    if (fused) {
      k_margi_erase_all<<<gl * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(nlev, thread_num, m, w.list1, w.rc, gate);
    } else {
      for (int L = nlev - 1; L >= 1; L--)
        k_margi_internal<<<gl * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(L, thread_num, m, w.list1, w.rc, gate);
      for (int L = 0; L < nlev; L++)
        k_margi_erase_mark<<<gl * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(L, thread_num, m, w.list1, w.rc, gate);
      k_clear_mark<<<gl, kBlock, 0, s>>>(nlev - 2, nlev, thread_num, m, w.list1, w.rc, gate);
    }
    // slide list compaction, the device-state slide, the counter publication
    k_slide_compact<<<1, 1024, 0, s>>>(thread_num, m, ctx->st, wa.win_count, mp.W - 1, ctx->d_pub, -1, gate);
    VG_HIP(hipGetLastError());
    return VG_OK;
  };
  (void)n_oldest;
  if (!ctx->use_graphs || ctx->prof_stages) return body();
  hipGraphExec_t& ge = ctx->g_margi[(gate ? 1 : 0) + (copy_signals ? 2 : 0)];
  VG_TRY(capture_once(ctx, s, &ge, body));
  VG_HIP(hipGraphLaunch(ge, s));
  return VG_OK;  // device error flags reach the host with the end-of-scan counters
}

// The margi tail inside the scan graph (pipeline.cpp stage_insert_recut),
// captured on the context stream behind the first two LM iterations: gated on
// the LM's `fin` like a speculative tail; the margi prefix (second stream) is
// waited for on a device flag (d_sync[4] >= DState::ph[4], by k_margi_leaf's
// leaf workgroups: no polling kernel in front); the publication
// numbers come from DState::ph; the ring (wa) is the graph's own.
int map_margi_tail_capture(vg_ctx* ctx, const MP& mp, const WinArg& wa) {
  DevMap& m = ctx->map;
  Work& w = ctx->wk;
  hipStream_t s = ctx->stream;
  const int nlev = mp.max_layer + 1;
  WinD* dwin = (WinD*)ctx->ba.xs;
  int* dn = (int*)((char*)ctx->ba.xs + sizeof(WinD));
  const int* gate = ba_gate_dev(ctx);
  const int thread_num = ctx->cfg.thread_num;
  k_margi_leaf<<<1 + 512 * kBlock / kSpreadBlock, kSpreadBlock, 0, s>>>(
      m.counters + kCntLeaves, w.list0, mp, wa, ctx->st, dwin, dn, dn + 32, 1, ba_iters_dev(ctx), ba_hess_dev(ctx),
      ctx->d_pub, 0, m, ctx->ba.fac_eig, ctx->ba.fac_pcr, w.plan, gate, ctx->d_sync + 2, ctx->margi_batch ? 1 : 0,
      &ctx->st->ph[1], ctx->d_sync + 4, 0);  // (no scan graph while the markers are on, scan_graph_ok)
  k_margi_copy<<<256, 64 * kCopyWaves, 0, s>>>(m.counters + kCntLeaves, w.plan, dwin, m, gate, w.list0,
                                                ctx->margi_fused ? 1 : 0, ctx->d_sync, ctx->st);
  if (ctx->margi_fused) {
    k_margi_erase_all<<<64 * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(nlev, thread_num, m, w.list1, w.rc, gate);
  } else {
    for (int L = nlev - 1; L >= 1; L--)
      k_margi_internal<<<64 * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(L, thread_num, m, w.list1, w.rc, gate);
    for (int L = 0; L < nlev; L++)
      k_margi_erase_mark<<<64 * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(L, thread_num, m, w.list1, w.rc, gate);
    k_clear_mark<<<64, kBlock, 0, s>>>(nlev - 2, nlev, thread_num, m, w.list1, w.rc, gate);
  }
  k_slide_compact<<<1, 1024, 0, s>>>(thread_num, m, ctx->st, wa.win_count, mp.W - 1, ctx->d_pub, -1, gate);
  VG_HIP(hipGetLastError());
  return VG_OK;
}

}  // namespace vg

#ifdef VG_PROBE
VG_PROBE_READER(vg_probe_read_margi)
#endif
