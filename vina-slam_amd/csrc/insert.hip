// insert.hip — a scan's points into the device-resident voxel map (map.hip).
//
// SURVEY §8(a) rows:
//   A3  var_init / pvec_update           point_utils.cpp:3-65        (fused)
//   A4  cut_voxel_multi -> allocate/push voxel_map.cpp:47-135, octree.cpp:151-228
#include <cstring>
#include <vector>
#include "vg_map.h"

namespace vg {

// ------------------------------------------------------------------ insert (A3/A4)
// per downsampled point: var_init + pvec_update (world var), world point, root
// key insert-or-find, first-occurrence marking of brand-new keys.
// kPre (the initialisation's cut_voxel, initialization.cpp:229-246): body
// points already motion-compensated (pin, fp64), the pose and covariance of
// x_buf[i] in xsrc (kXC layout), and either the identity body covariance
// without pvec_update (var_identity, rounds before convergence) or calcBodyVar
// on the body point + pvec_update.
template <bool kPre>
__global__ void __launch_bounds__(256) k_ins_prep(int n_arg, const int* __restrict__ nd, const float* __restrict__ ox, const float* __restrict__ oy,
                           const float* __restrict__ oz, const float* __restrict__ oi, MP mp, DState* __restrict__ st, int slot,
                           DevMap m, double* __restrict__ pw, uint32_t* __restrict__ hslot,
                           const PushArg* __restrict__ pa, const double* __restrict__ pin, const double* __restrict__ xsrc,
                           int var_identity, int* __restrict__ dsf, unsigned long long* __restrict__ gran, int ngran,
                           const int* __restrict__ ph_in) {
  const int n = nd ? *nd : n_arg;  // the downsampled count on the device (ds_enqueue_hashed)
  {  // the root registration's look-back granules (k_ins_roots_lb, the next launch) start empty
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (gran && g < ngran) gran[g] = 0ull;
  }
  // the window push (local_mapping.cpp:434-441) rides in block 0: it copies
  // x_curr into x_buf[ord], which this kernel only reads
  if (!kPre && pa && blockIdx.x == 0) push_state_block(st, *pa);  // pa: host-mapped (vg_ctx::d_in)
  // the scan graph's per-scan numbers (HostIn::ph, host-mapped) into the device state, beside the push
  if (ph_in && blockIdx.x == 0 && threadIdx.x < 6) st->ph[threadIdx.x] = ph_in[threadIdx.x];
  // pose of x_buf[ord] = x_curr after the IEKF (device state)
  const double* xc = kPre ? xsrc : st->xc;
  M3 R, rot_var, tsl_var;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      R(r, c) = xc[r * 3 + c];
      rot_var(r, c) = xc[kXS + r * 15 + c];
      tsl_var(r, c) = xc[kXS + (3 + r) * 15 + 3 + c];
    }
  const V3 p = ld_v3(xc + 9);
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // per-insert device counters (read by the later kernels)
    m.counters[kCntNew] = m.counters[kCntNodes];  // first id of this scan's new roots
    m.counters[kCntSlideBase] = m.counters[kCntSlide];  // surf_map_slide size before this scan's roots
    m.counters[kCntTouched] = 0;
    m.counters[kCntCreate] = 0;
    m.counters[kCntSeg] = 0;
    m.counters[kCntSegCur] = 0;
    m.counters[kCntMisc] = 0;  // insert abort flag (child-allocation overflow)
    m.counters[kCntPlaneUpd] = 0;  // margi's per-scan branch counters (vg_stats)
    m.counters[kCntFixFull] = 0;
    m.counters[kCntNds] = n;
    m.wpn[slot] = n;  // window points of this physical slot (k_make_win)
    m.slot_epoch[slot] += 1;  // every leaf run of the slot's previous scan is stale now
    m.arena[slot] = m.cap_wp;
    if (dsf && dsf[0]) {  // the downsample's key-range error (no host wait in between)
      atomicOr(&m.counters[kCntErr], 1);
      dsf[0] = 0;
    }
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    V3 pnt;
    M3 vw;
    if (kPre) {
      pnt = v3(pin[(size_t)i * 3], pin[(size_t)i * 3 + 1], pin[(size_t)i * 3 + 2]);
      if (var_identity) {
        vw = M3::I();
      } else {
        const M3 var = calc_body_var(pnt, mp.dept, mp.beam_dv);
        vw = world_var(R, var, pnt, rot_var, tsl_var);
      }
    } else {
      M3 var;
      var_init_pt(mp, ox[i], oy[i], oz[i], pnt, var);
      vw = world_var(R, var, pnt, rot_var, tsl_var);
    }
    V3 w = rigid(R, pnt, p);
    size_t base = (size_t)slot * m.cap_wp + i;
    for (int j = 0; j < 3; j++) m.wp_pnt[base * 3 + j] = pnt[j];
    for (int j = 0; j < 9; j++) m.wp_var[base * 9 + j] = vw[j];
    m.wp_leaf[base] = -1;
    m.wp_int[base] = oi ? oi[i] : 0.f;
    for (int j = 0; j < 3; j++) pw[(size_t)i * 3 + j] = w[j];
    uint64_t key;
    if (!pack_key(w, mp.vs, key)) {
      atomicOr(&m.counters[kCntErr], 1);
      hslot[i] = 0xffffffffu;
      continue;
    }
    if (!owns(m, key)) {  // another shard's tile (sharded mode)
      hslot[i] = 0xffffffffu;
      continue;
    }
    bool fresh;
    int s = hash_insert(m.hkey, m.hash_mask, key, fresh);
    if (s < 0) {
      atomicOr(&m.counters[kCntErr], 2);
      hslot[i] = 0xffffffffu;
      continue;
    }
    hslot[i] = (uint32_t)s;
    atomicMin(&m.hfirst[s], i);  // the root's first point this scan (k_ins_flags)
  }
}

// Root registration of cut_voxel_multi (voxel_map.cpp:57-90) in two launches
// (flags + per-tile ranks, then allocation), replacing a flag / scan /
// allocate / count / zero / touch chain. Points are taken in index tiles of
// kRootTile; a point is its root's first point this scan iff hfirst[slot] == i
// (k_ins_prep). Per tile: how many first points, new roots, and roots joining
// surf_map_slide (new ones, and existing ones not yet in it), with each
// point's rank inside its tile. Ids and slide positions then follow point
// index order: deterministic.
constexpr int kRootTile = 1024;  // points per workgroup (256 threads x 4)
__device__ __forceinline__ int ins_root_code(const DevMap& m, const uint32_t* __restrict__ hslot, int i, int n) {
  // bit 0: first point of its root, bit 1: new root, bit 2: joins the slide map
  if (i >= n) return 0;
  const uint32_t s = hslot[i];
  if (s == 0xffffffffu || m.hfirst[s] != i) return 0;
  const int r = m.hval[s];
  if (r < 0) return 7;
  return m.in_slide[r] ? 1 : 5;
}
// exclusive block scan of three counts packed 3 x 21 bits
typedef unsigned long long u64;
__device__ __forceinline__ u64 pack3(int code) {
  return (u64)(code & 1) | ((u64)((code >> 1) & 1) << 21) | ((u64)((code >> 2) & 1) << 42);
}
__device__ __forceinline__ u64 block_excl_scan3(u64 v, u64* s_w, u64* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  u64 x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const u64 y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) s_w[wv] = x;
  __syncthreads();
  u64 base = 0, tot = 0;
  for (int k = 0; k < nw; k++) {
    if (k < wv) base += s_w[k];
    tot += s_w[k];
  }
  __syncthreads();
  *total = tot;
  return base + x - v;
}
__global__ void __launch_bounds__(256) k_ins_flags(int n_arg, const int* __restrict__ nd, const uint32_t* __restrict__ hslot, DevMap m,
                                                   uint32_t* __restrict__ rank, int* __restrict__ tile_cnt) {
  const int n = nd ? *nd : n_arg;  // the downsampled count on the device (ds_enqueue_hashed)
  __shared__ u64 s_w[4];
  const int i0 = blockIdx.x * kRootTile + threadIdx.x * 4;
  int code[4];
  u64 v = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    code[k] = ins_root_code(m, hslot, i0 + k, n);
    v += pack3(code[k]);
  }
  u64 tot;
  u64 r = block_excl_scan3(v, s_w, &tot);
  constexpr u64 kF = (1ull << 21) - 1;
#pragma unroll
  for (int k = 0; k < 4; k++) {  // rank: new-root rank | slide rank << 16 (< 1024 each), code in the top bits
    if (i0 + k < n)
      rank[i0 + k] = (unsigned)((r >> 21) & kF) | ((unsigned)((r >> 42) & kF) << 16) | ((unsigned)code[k] << 29);
    r += pack3(code[k]);
  }
  if (threadIdx.x == 0) {
    tile_cnt[blockIdx.x * 3 + 0] = (int)(tot & kF);
    tile_cnt[blockIdx.x * 3 + 1] = (int)((tot >> 21) & kF);
    tile_cnt[blockIdx.x * 3 + 2] = (int)((tot >> 42) & kF);
  }
}
// new roots at kCntNew + (new roots of earlier tiles) + rank, centre
// (0.5 + k) voxel_size, records zeroed; existing first-touched roots isexist
// (voxel_map.cpp:70); slide appends in point order; the root counters. The
// point -> root lookup itself is left to k_ins_descend (after this launch).
__global__ void __launch_bounds__(256) k_ins_roots_alloc(int n_arg, const int* __restrict__ nd, int ntile, const uint32_t* __restrict__ hslot,
                                                         const uint32_t* __restrict__ rank,
                                                         const int* __restrict__ tile_cnt, MP mp, DevMap m) {
  const int n = nd ? *nd : n_arg;  // the downsampled count on the device (ds_enqueue_hashed)
  __shared__ int s_red[3][4];
  int a[3] = {0, 0, 0}, t[3] = {0, 0, 0};
  for (int b = threadIdx.x; b < ntile; b += blockDim.x)
    for (int j = 0; j < 3; j++) {
      const int c = tile_cnt[b * 3 + j];
      t[j] += c;
      if (b < (int)blockIdx.x) a[j] += c;
    }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int off[3], tot[3];
  for (int j = 0; j < 3; j++) {  // (a: this tile's offset, t: the totals) over the block
    int x = a[j], y = t[j];
    for (int o = 32; o > 0; o >>= 1) {
      x += __shfl_down(x, o, 64);
      y += __shfl_down(y, o, 64);
    }
    if (lane == 0) s_red[j][wv] = x;
    __syncthreads();
    off[j] = s_red[j][0] + s_red[j][1] + s_red[j][2] + s_red[j][3];
    __syncthreads();
    if (lane == 0) s_red[j][wv] = y;
    __syncthreads();
    tot[j] = s_red[j][0] + s_red[j][1] + s_red[j][2] + s_red[j][3];
    __syncthreads();
  }
  const int base = m.counters[kCntNew], sbase = m.counters[kCntSlideBase];
  const int i0 = blockIdx.x * kRootTile;
  for (int i = i0 + threadIdx.x; i < min(n, i0 + kRootTile); i += blockDim.x) {
    const uint32_t rk = rank[i];
    const int code = (int)(rk >> 29);
    if (!(code & 1)) continue;
    const uint32_t s = hslot[i];
    int r;
    if (code & 2) {  // a new root (voxel_map.cpp:77-83): centre, quater_length, empty records
      r = base + off[1] + (int)(rk & 0xffffu);
      if (r >= m.cap_nodes) {
        atomicOr(&m.counters[kCntErr], 4);
        continue;
      }
      const uint64_t key = m.hkey[s];
      double c[3];
      const int64_t k[3] = {unpack_axis(key, 42), unpack_axis(key, 21), unpack_axis(key, 0)};
      for (int j = 0; j < 3; j++) c[j] = (0.5 + k[j]) * mp.vs;
      init_node(m.hdr[r], c, (float)(mp.vs / 4.0), 0, -1);  // records zeroed by map_reset
      dbox_root(m.dbox + (size_t)r * 6);
      m.hval[s] = r;
    } else {
      r = m.hval[s];
      m.hdr[r].isexist = 1;
    }
    if (code & 4) {
      m.in_slide[r] = 1;
      m.slide[sbase + off[2] + (int)((rk >> 16) & 0x1fffu)] = r;
    }
    m.hfirst[s] = 0x7f7f7f7f;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    m.counters[kCntNodes] = min(base + tot[1], m.cap_nodes);
    m.counters[kCntRoots] = tot[1];
    m.counters[kCntTouched] = tot[0];
    m.counters[kCntSlide] = sbase + tot[2];
  }
}

// Root registration in ONE launch (k_ins_flags + k_ins_roots_alloc): each
// 1024-point tile publishes its three counts (first points, new roots, slide
// joiners) as one 64-bit granule {valid bit, 3 x 21-bit counts} with an
// agent-scope store, then sums the granules of the tiles before it (decoupled
// look-back: tiles are dispatched in order per XCD, so a tile only ever waits
// for tiles already dispatched) and allocates its own roots at base + prefix —
// the same ids and slide positions as the two-launch form. The granules are
// zeroed by k_ins_prep, the launch before. The last tile writes the totals.
__global__ void __launch_bounds__(256) k_ins_roots_lb(int n_arg, const int* __restrict__ nd, int ntile,
                                                      const uint32_t* __restrict__ hslot, MP mp, DevMap m,
                                                      unsigned long long* __restrict__ gran) {
  const int n = nd ? *nd : n_arg;
  __shared__ u64 s_w[4];
  __shared__ int s_off[3], s_tot[3];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const int i0 = b * kRootTile + tid * 4;
  int code[4];
  u64 v = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    code[k] = ins_root_code(m, hslot, i0 + k, n);
    v += pack3(code[k]);
  }
  u64 tot;
  u64 r = block_excl_scan3(v, s_w, &tot);
  constexpr u64 kF = (1ull << 21) - 1;
  if (tid == 0) __hip_atomic_store(&gran[b], tot | (1ull << 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid < 64) {  // wave 0: the earlier tiles' counts (and, in the last tile, everyone's)
    const bool last = b == ntile - 1;
    const int upto = last ? ntile : b;
    int a0 = 0, a1 = 0, a2 = 0, t0 = 0, t1 = 0, t2 = 0;
    for (int k = lane; k < upto; k += 64) {
      u64 g;
      for (long it = 0;; it++) {
        g = __hip_atomic_load(&gran[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g >> 63) break;
        __builtin_amdgcn_s_sleep(1);
        if (it > (1l << 24)) {  // never: a tile that never publishes (bounded, not a hang)
          atomicOr(&m.counters[kCntErr], 64);
          g = 1ull << 63;
          break;
        }
      }
      const int c0 = (int)(g & kF), c1 = (int)((g >> 21) & kF), c2 = (int)((g >> 42) & kF);
      if (k < b) {
        a0 += c0;
        a1 += c1;
        a2 += c2;
      }
      t0 += c0;
      t1 += c1;
      t2 += c2;
    }
    for (int o = 32; o > 0; o >>= 1) {
      a0 += __shfl_down(a0, o, 64);
      a1 += __shfl_down(a1, o, 64);
      a2 += __shfl_down(a2, o, 64);
      t0 += __shfl_down(t0, o, 64);
      t1 += __shfl_down(t1, o, 64);
      t2 += __shfl_down(t2, o, 64);
    }
    if (lane == 0) {
      s_off[0] = a0;
      s_off[1] = a1;
      s_off[2] = a2;
      s_tot[0] = t0;
      s_tot[1] = t1;
      s_tot[2] = t2;
    }
  }
  __syncthreads();
  const int base = m.counters[kCntNew], sbase = m.counters[kCntSlideBase];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int i = i0 + k;
    const int cd = code[k];
    const u64 rk = r;
    r += pack3(cd);
    if (i >= n || !(cd & 1)) continue;
    const uint32_t s = hslot[i];
    int rt;
    if (cd & 2) {  // a new root (voxel_map.cpp:77-83): centre, quater_length, empty records
      rt = base + s_off[1] + (int)((rk >> 21) & kF);
      if (rt >= m.cap_nodes) {
        atomicOr(&m.counters[kCntErr], 4);
        continue;
      }
      const uint64_t key = m.hkey[s];
      double c[3];
      const int64_t kk[3] = {unpack_axis(key, 42), unpack_axis(key, 21), unpack_axis(key, 0)};
      for (int j = 0; j < 3; j++) c[j] = (0.5 + kk[j]) * mp.vs;
      init_node(m.hdr[rt], c, (float)(mp.vs / 4.0), 0, -1);  // records zeroed by map_reset
      dbox_root(m.dbox + (size_t)rt * 6);
      m.hval[s] = rt;
    } else {
      rt = m.hval[s];
      m.hdr[rt].isexist = 1;
    }
    if (cd & 4) {
      m.in_slide[rt] = 1;
      m.slide[sbase + s_off[2] + (int)((rk >> 42) & kF)] = rt;
    }
    m.hfirst[s] = 0x7f7f7f7f;
  }
  if (b == ntile - 1 && tid == 0) {
    m.counters[kCntNodes] = min(base + s_tot[1], m.cap_nodes);
    m.counters[kCntRoots] = s_tot[1];
    m.counters[kCntTouched] = s_tot[0];
    m.counters[kCntSlide] = sbase + s_tot[2];
  }
}

// the later insert kernels do nothing when the scan touched fewer than
// thread_num roots (voxel_map.cpp:96-97: no allocation at all) or when the
// child allocation overflowed k_ins_alloc (the host replays them)
__device__ __forceinline__ bool ins_skip(const DevMap& m, int thread_num) {
  return g_touched(m) < thread_num || m.counters[kCntMisc] != 0;
}

// descend to a leaf; a missing child becomes a creation request (parent, octant).
// leaf[i]: the leaf, -1 (no root) or the request's code -2 - (parent * 8 + octant).
// kCount: the point is counted into its bucket here — m.leaf_cnt[leaf] at an
// existing leaf, m.creq_cnt[parent * 8 + octant] at a request (a child made by
// alloc_parent is always a leaf) — and the bucket's first point (the first
// arrival at the leaf, the request's CAS winner) appends its segment:
// seg_key[s] = leaf[i]. Every segment's length is final when this launch
// ends, so no later pass has to count (k_ins_resolve) and the offsets need no
// ordered prefix (k_seg_offsets): k_ins_alloc_seg hands them out in any order.
template <bool kCount>
__global__ void __launch_bounds__(256) k_ins_descend(int n_arg, const int* __restrict__ nd, int thread_num, const double* __restrict__ pw, DevMap m,
                                                     const uint32_t* __restrict__ hslot, int* __restrict__ leaf,
                                                     int* __restrict__ reqlist, int* __restrict__ seg_key) {
  const int n = nd ? *nd : n_arg;  // the downsampled count on the device (ds_enqueue_hashed)
  if (ins_skip(m, thread_num)) return;
  for (int base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
    const int i = base + threadIdx.x;
    int node = -1;
    bool first = false;
    if (i < n) {
      const uint32_t hs = hslot[i];
      node = hs != 0xffffffffu ? m.hval[hs] : -1;  // the point's root (registered by k_ins_roots_alloc)
    }
    if (node >= 0) {
      V3 w = v3(pw[3 * i], pw[3 * i + 1], pw[3 * i + 2]);
      for (int d = 0; d < 8; d++) {
        const NodeHdr& h = m.hdr[node];
        if (h.octo == 0) break;
        int o = octant(w, h.center);
        int c = h.child[o];
        if (c < 0) {
          // request (parent, octant); the first requester of a parent registers it
          if (atomicCAS(&m.cfirst[(size_t)node * 8 + o], 0x7f7f7f7f, -5) == 0x7f7f7f7f) {
            first = true;
            if (atomicExch(&m.nscr[(size_t)node * 4 + 1], -7) != -7) {
              int pos = atomicAdd(&m.counters[kCntCreate], 1);
              reqlist[pos] = node;
            }
          }
          if (kCount) atomicAdd(&m.creq_cnt[(size_t)node * 8 + o], 1);
          node = -2 - (node * 8 + o);
          break;
        }
        node = c;
      }
      if (kCount && node >= 0) first = atomicAdd(&m.leaf_cnt[node], 1) == 0;
    }
    if (i < n) leaf[i] = node;
    if (kCount) {
      const int s = wave_append(&m.counters[kCntSeg], first ? 1 : 0);
      if (first) seg_key[s] = node;
    }
  }
}

// the final leaf of every point, and its bucket: a point count per leaf
// (m.leaf_cnt, zero between inserts) and, for the leaf's first point, a
// segment (seg_leaf[s] = leaf, m.leaf_seg[leaf] = s). Segment order is free:
// k_push_window treats every leaf on its own; only the order of a leaf's
// points matters, and k_push_window restores it.
__global__ void __launch_bounds__(256) k_ins_resolve(int n_arg, const int* __restrict__ nd, int thread_num, const double* __restrict__ pw, DevMap m,
                                                     int* __restrict__ leaf, int* __restrict__ seg_leaf) {
  const int n = nd ? *nd : n_arg;  // the downsampled count on the device (ds_enqueue_hashed)
  if (ins_skip(m, thread_num)) return;
  for (int base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
    const int i = base + threadIdx.x;
    int node = i < n ? leaf[i] : -1;
    if (node < -1) {
      const int code = -2 - node;
      node = m.hdr[code >> 3].child[code & 7];
      leaf[i] = node;
    }
    const bool first = node >= 0 && atomicAdd(&m.leaf_cnt[node], 1) == 0;
    const int s = wave_append(&m.counters[kCntSeg], first ? 1 : 0);
    if (first) {
      seg_leaf[s] = node;
      m.leaf_seg[node] = s;
    }
  }
}

// one workgroup: segment offsets = prefix over the segments' point counts;
// the counts return to zero (k_ins_scatter counts the fill again)
__global__ void __launch_bounds__(1024) k_seg_offsets(int thread_num, DevMap m, const int* __restrict__ seg_leaf,
                                                      int* __restrict__ seg_off) {
  __shared__ int s_w[17];
  if (ins_skip(m, thread_num)) return;
  const int ns = m.counters[kCntSeg];
  const int per = (ns + (int)blockDim.x - 1) / (int)blockDim.x;
  const int s0 = threadIdx.x * per, s1 = min(ns, s0 + per);
  constexpr int kPer = 32;
  int total;
  if (per <= kPer) {  // all loads of a lane issued before any is used (two round trips, not 2 per segment)
    int lf[kPer], c[kPer];
#pragma unroll
    for (int k = 0; k < kPer; k++) lf[k] = s0 + k < s1 ? seg_leaf[s0 + k] : -1;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
      c[k] = lf[k] >= 0 ? m.leaf_cnt[lf[k]] : 0;
      cnt += c[k];
    }
    int pos = block_excl_scan(cnt, s_w, &total);
#pragma unroll
    for (int k = 0; k < kPer; k++)
      if (lf[k] >= 0) {
        seg_off[s0 + k] = pos;
        pos += c[k];
        m.leaf_cnt[lf[k]] = 0;
      }
  } else {
    int cnt = 0;
    for (int q = s0; q < s1; q++) cnt += m.leaf_cnt[seg_leaf[q]];
    int pos = block_excl_scan(cnt, s_w, &total);
    for (int q = s0; q < s1; q++) {
      const int l = seg_leaf[q];
      seg_off[q] = pos;
      pos += m.leaf_cnt[l];
      m.leaf_cnt[l] = 0;
    }
  }
  if (threadIdx.x == 0) seg_off[ns] = total;
}

// every point into its segment (arbitrary order inside it)
__global__ void __launch_bounds__(256) k_ins_scatter(int n_arg, const int* __restrict__ nd, int thread_num, DevMap m, const int* __restrict__ leaf,
                                                     const int* __restrict__ seg_off, int* __restrict__ order) {
  const int n = nd ? *nd : n_arg;  // the downsampled count on the device (ds_enqueue_hashed)
  if (ins_skip(m, thread_num)) return;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int l = leaf[i];
    if (l < 0) continue;
    order[seg_off[m.leaf_seg[l]] + atomicAdd(&m.leaf_cnt[l], 1)] = i;
  }
}

// pvec_update into the leaves (voxel_map.cpp:104-131 / octree.cpp:151-177):
// one wave per leaf segment (k_ins_resolve / k_seg_offsets / k_ins_scatter);
// lanes 0-8 own the frame cluster, 9-17 the accumulated cluster, 18-62
// cov_add (see role_inc)
constexpr int kPushWaves = 4;
constexpr int kPwBits = 1 << 16;  // point indices per bitmap window of k_push_window (8 KB, inside the wave's E)
constexpr int kPwWords = kPwBits / 32;
constexpr int kPwRankMax = 256;  // longest segment ordered by ranking (the bitmap's cost is its index range)
static_assert(kPwWords * 4 <= 64 * kErec * 8, "the ordering bitmap lives in the wave's record buffer");
// the recut's head (k_make_win_recut_begin's work) riding in the insert's
// last launch as one extra workgroup: the window view and the level counters
// need only the insert's counts, and the recut's first level starts one launch
// boundary earlier (the insert + recut graph, map_insert's rb)
struct RcBeginArg {
  WinArg wa;
  DState* st;
  const int* wpn;
  WinD* win;
  int* nper;
  int* slot_of;
  int* rc;
};
// a segment's bucket count: per leaf, or per child request (k_ins_descend<true>)
__device__ __forceinline__ int* seg_counter(const DevMap& m, int key) {
  return key >= 0 ? &m.leaf_cnt[key] : &m.creq_cnt[-2 - key];
}
// kCur: the counted descent's hand-off — seg_leaf[s] is the segment's key (a
// leaf, or a request whose child the allocation has made by now) and seg_off
// holds (offset, length) pairs (k_ins_alloc_seg); else seg_off[s], seg_off[s + 1]
// bracket the segment (k_seg_offsets).
// kPipe: the records of a long segment's next 64 points are loaded into
// registers ahead of the current block's serial sums (the sums' order is the
// same), and a mid-size segment is ranked from a copy of its indices in LDS.
template <bool kCur, bool kPipe>
__global__ void __launch_bounds__(64 * kPushWaves, 4) k_push_window(const int* __restrict__ seg_leaf,
                                                                 const int* __restrict__ seg_off,
                                                                 const int* __restrict__ order,
                                                                 int* __restrict__ order2, MP mp, int slot, DevMap m,
                                                                 const double* __restrict__ pw, int thread_num,
                                                                 RcBeginArg rb, int has_rb) {
  __shared__ double E[kPushWaves][64][kErec];
  if (has_rb && blockIdx.x == gridDim.x - 1) {
    make_win_block(rb.st, rb.wa, rb.wpn, rb.win, rb.nper, rb.slot_of);
    __syncthreads();
    recut_begin_block(m, rb.rc, thread_num);
    return;
  }
  if (ins_skip(m, thread_num)) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int role = lane < 63 ? lane : -1;
  RoleIdx ri = role < 9 ? role_clu(role < 0 ? 0 : role, kEq) : role < 18 ? role_clu(role - 9, kEp) : role_cov(role - 18);
  const int nseg = m.counters[kCntSeg];
  const int gsz = (int)gridDim.x - (has_rb ? 1 : 0);
  for (int sg = blockIdx.x * kPushWaves + wv; sg < nseg; sg += gsz * kPushWaves) {
    int j0, L, leaf;
    int* bucket;  // the bucket's count, back to zero at the end (the bucketing invariant)
    if (kCur) {
      const int2 ol = reinterpret_cast<const int2*>(seg_off)[sg];
      const int key = seg_leaf[sg];
      j0 = ol.x;
      L = ol.y;
      bucket = seg_counter(m, key);
      leaf = key >= 0 ? key : m.hdr[(-2 - key) >> 3].child[(-2 - key) & 7];
      if (leaf < 0) {  // the child was not made (node pool full, kCntErr): nothing to push into
        if (lane == 0) *bucket = 0;
        continue;
      }
    } else {
      j0 = seg_off[sg];
      L = seg_off[sg + 1] - j0;
      leaf = seg_leaf[sg];
      bucket = &m.leaf_cnt[leaf];
    }
    // the leaf's points in index order (the reference's push order): up to 64
    // sorted across the lanes (bitonic by xor shuffles), longer segments ranked
    // into order2
    int mine = lane < L ? order[j0 + lane] : 0x7fffffff;
    if (L <= 64) {
#pragma unroll
      for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
          const int other = __shfl_xor(mine, j, 64);
          const bool up = (lane & k) == 0, low = (lane & j) == 0;
          mine = (low == up) ? min(mine, other) : max(mine, other);
        }
    } else if (kPipe && L <= kPwRankMax) {  // a few hundred points: each ranked against the others, staged in LDS
      int* idx = reinterpret_cast<int*>(&E[wv][0][0]);  // free until the records are filled
      for (int e = lane; e < L; e += 64) idx[e] = order[j0 + e];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      for (int e = lane; e < L; e += 64) {
        const int x = idx[e];
        int r = 0;
        for (int t = 0; t < L; t++) r += idx[t] < x ? 1 : 0;
        order2[j0 + r] = x;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else if (L <= kPwRankMax) {  // a few hundred points: each ranked against the (L1-resident) others
      for (int e = lane; e < L; e += 64) {
        const int x = order[j0 + e];
        int r = 0;
        for (int t = 0; t < L; t++) r += order[j0 + t] < x ? 1 : 0;
        order2[j0 + r] = x;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
      // longer segments: an LDS bitmap over the segment's index range, in
      // windows of kPwBits indices (set bits compacted in order by a wave
      // scan): O(L + range / 32) per leaf instead of ranking every point
      // against every other (O(L^2 / 64) global loads per lane)
      uint32_t* bm = reinterpret_cast<uint32_t*>(&E[wv][0][0]);  // free until the records are filled
      int lo = 0x7fffffff, hi = -1;
      for (int e = lane; e < L; e += 64) {
        const int x = order[j0 + e];
        lo = min(lo, x);
        hi = max(hi, x);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
      }
      int outpos = 0;
      for (int w0 = lo; w0 <= hi; w0 += kPwBits) {
        const int nw = min(kPwWords, ((hi - w0) >> 5) + 1);  // the words this window's range covers
        for (int k = lane; k < nw; k += 64) bm[k] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        for (int e = lane; e < L; e += 64) {
          const int off = order[j0 + e] - w0;
          if (off >= 0 && off < kPwBits) atomicOr(&bm[off >> 5], 1u << (off & 31));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // 64 consecutive words per round, one per lane: a lane emits at
        // most 32 indices per round however the points cluster
        for (int r = 0; r < nw; r += 64) {
          const int k = r + lane;
          uint32_t w = k < nw ? bm[k] : 0u;
          const int cnt = __popc(w);
          int ex = cnt;
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(ex, off, 64);
            if (lane >= off) ex += y;
          }
          int pos = outpos + ex - cnt;
          while (w) {
            const int b = __ffs(w) - 1;
            w &= w - 1;
            order2[j0 + pos++] = w0 + k * 32 + b;
          }
          outpos += __shfl(ex, 63, 64);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      }
    }
    const bool listed = m.hdr[leaf].layer < mp.max_layer;
    if (listed) {  // the leaf's run of this slot (index order), for the recut's subdivisions and the margi
      int* ord = m.wp_ord + (size_t)slot * m.ord_stride + j0;
      if (L <= 64) {
        if (lane < L) ord[lane] = mine;
      } else {
        for (int e = lane; e < L; e += 64) ord[e] = order2[j0 + e];
      }
      if (lane == 0) m.lseg[(size_t)leaf * mp.W + slot] = lseg_pack(j0, L, m.slot_epoch[slot]);
    }
    Clu* loc = &m.pcrs[(size_t)leaf * mp.W + slot];
    Clu* add = &m.pcr_add[leaf];
    double* acc_p = role < 0 ? nullptr
                    : role < 9 ? (role < 6 ? &loc->P[role] : &loc->v[role - 6])
                    : role < 18 ? (role < 15 ? &add->P[role - 9] : &add->v[role - 15])
                                : &m.cov_add[(size_t)leaf * kCovN + role - 18];
    double acc = acc_p ? *acc_p : 0.0;
    if (kPipe && L > 64) {
      // the next block's record loads (15 doubles a lane, each dependent on
      // order2) are in flight while this block's 64 ordered adds run
      V3 q, p;
      M3 V;
      auto load = [&](int base) {
        const int e = base + lane;
        if (e < L) {
          const int i = order2[j0 + e];
          const size_t b = (size_t)slot * m.cap_wp + i;
          q = ld_v3(&m.wp_pnt[b * 3]);
          p = v3(pw[3 * i], pw[3 * i + 1], pw[3 * i + 2]);
          V = ld_m3(&m.wp_var[b * 9]);
          if (listed) m.wp_leaf[b] = leaf;
        }
      };
      load(0);
      for (int base = 0; base < L; base += 64) {
        if (base + lane < L) fill_record(E[wv][lane], q, p, V);
        const int nb = min(64, L - base);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        load(base + 64);
#pragma unroll 8
        for (int k = 0; k < nb; k++) acc += role_inc(E[wv][k], ri);
        __builtin_amdgcn_wave_barrier();
      }
    } else {
      for (int base = 0; base < L; base += 64) {
        const int e = base + lane;
        const bool valid = e < L;
        if (valid) {
          const int i = L <= 64 ? mine : order2[j0 + e];
          const size_t b = (size_t)slot * m.cap_wp + i;
          fill_record(E[wv][lane], ld_v3(&m.wp_pnt[b * 3]), v3(pw[3 * i], pw[3 * i + 1], pw[3 * i + 2]),
                      ld_m3(&m.wp_var[b * 9]));
          if (listed) m.wp_leaf[b] = leaf;
        }
        const int nb = min(64, L - base);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 8
        for (int k = 0; k < nb; k++) acc += role_inc(E[wv][k], ri);  // unrolled: the LDS reads run ahead of the sum
        __builtin_amdgcn_wave_barrier();
      }
    }
    if (acc_p) *acc_p = acc;
    if (lane == 0) {
      loc->N += L;
      add->N += L;
      m.hdr[leaf].has_sw = 1;
      m.hdr[leaf].isexist = 1;
      *bucket = 0;  // bucketing invariant: zero between inserts
    }
  }
}

// ascending bitonic sort of n (power of two) keys in LDS by the whole workgroup
template <typename T>
__device__ void lds_bitonic(T* a, int n) {
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int pj = i ^ j;
        if (pj > i) {
          const T x = a[i], y = a[pj];
          const bool up = (i & k) == 0;
          if ((x > y) == up) {
            a[i] = y;
            a[pj] = x;
          }
        }
      }
      __syncthreads();
    }
}

// children requested by k_ins_descend, in one workgroup: parents sorted
// ascending (deterministic ids), per-parent octant order, ids base + prefix,
// records zeroed. More than kInsAllocCap parents sets the abort flag and the
// host replays the allocation on the host-sized path.
constexpr int kInsAllocCap = 4096;
__device__ __forceinline__ void ins_alloc_block(int thread_num, DevMap& m, const int* __restrict__ reqlist, int cap,
                                                int* sp, int* s_w) {
  if (g_touched(m) < thread_num) return;
  const int np = m.counters[kCntCreate];
  if (np == 0) return;
  if (np > cap) {
    if (threadIdx.x == 0) m.counters[kCntMisc] = 1;
    return;
  }
  int npad = 2;
  while (npad < np) npad <<= 1;
  for (int i = threadIdx.x; i < npad; i += blockDim.x) sp[i] = i < np ? reqlist[i] : 0x7fffffff;
  __syncthreads();
  lds_bitonic(sp, npad);
  const int base = m.counters[kCntNodes];
  int carry = 0;
  for (int start = 0; start < np; start += blockDim.x) {
    const int q = start + threadIdx.x;
    const int p = q < np ? sp[q] : -1;
    int cc = 0;
    if (p >= 0)
      for (int o = 0; o < 8; o++) cc += (m.cfirst[(size_t)p * 8 + o] == -5) ? 1 : 0;
    int tot;
    const int off = block_excl_scan(cc, s_w, &tot);
    if (p >= 0) alloc_parent(m, p, base + carry + off, nullptr, 0);
    carry += tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) m.counters[kCntNodes] = base + carry;
}
__global__ void __launch_bounds__(1024) k_ins_alloc(int thread_num, DevMap m, const int* __restrict__ reqlist,
                                                    int cap) {
  __shared__ int sp[kInsAllocCap];
  __shared__ int s_w[17];
  ins_alloc_block(thread_num, m, reqlist, cap, sp, s_w);
}

// The child allocation (workgroup 0, as k_ins_alloc) and, beside it, the
// segment allocation of the counted descent (the other workgroups): a
// segment's place in the bucketed point order is a wave-aggregated atomicAdd
// of its length on one cursor — any order will do, k_push_window treats every
// leaf on its own. seg_ol[s] = (offset, length); the bucket's count becomes
// its fill cursor (k_ins_scatter_cur adds from there), so it holds offset +
// length after the scatter and k_push_window returns it to zero. The two
// halves share nothing: the segments need the counts only, not the children's
// ids (k_push_window resolves a request's child), and a child-allocation
// overflow (kCntMisc, raised in this launch) leaves the segments valid for
// map_insert_replay's tail.
constexpr int kSegAllocBlocks = 8;
__global__ void __launch_bounds__(1024) k_ins_alloc_seg(int thread_num, DevMap m, const int* __restrict__ reqlist,
                                                        int cap, const int* __restrict__ seg_key,
                                                        int2* __restrict__ seg_ol) {
  __shared__ int sp[kInsAllocCap];
  __shared__ int s_w[17];
  if (blockIdx.x == 0) {
    ins_alloc_block(thread_num, m, reqlist, cap, sp, s_w);
    return;
  }
  if (g_touched(m) < thread_num) return;  // (the descent did not run: no segments)
  const int ns = m.counters[kCntSeg];
  for (int base = ((int)blockIdx.x - 1) * (int)blockDim.x; base < ns; base += ((int)gridDim.x - 1) * (int)blockDim.x) {
    const int s = base + threadIdx.x;
    int* c = s < ns ? seg_counter(m, seg_key[s]) : nullptr;
    const int len = c ? *c : 0;
    const int off = wave_append(&m.counters[kCntSegCur], len);
    if (c) {
      seg_ol[s] = make_int2(off, len);
      *c = off;
    }
  }
}

// every point into its segment (arbitrary order inside it), counted descent:
// the bucket's counter is the segment's fill cursor (k_ins_alloc_seg)
__global__ void __launch_bounds__(256) k_ins_scatter_cur(int n_arg, const int* __restrict__ nd, int thread_num, DevMap m,
                                                         const int* __restrict__ leaf, int* __restrict__ order) {
  const int n = nd ? *nd : n_arg;  // the downsampled count on the device (ds_enqueue_hashed)
  if (ins_skip(m, thread_num)) return;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int l = leaf[i];
    if (l == -1) continue;
    order[atomicAdd(seg_counter(m, l), 1)] = i;
  }
}

// leaves -> sorted (leaf, order) keys -> pushes of one insert
static int insert_tail(vg_ctx* ctx, const MP& mp, int slot, int n, int thread_num, const int* nd = nullptr) {
  DevMap& m = ctx->map;
  Work& w = ctx->wk;
  hipStream_t s = ctx->stream;
  const int g = grid_for(n);
  const int gseg = (n + kPushWaves - 1) / kPushWaves < 2048 ? (n + kPushWaves - 1) / kPushWaves : 2048;
  int* seg_leaf = w.list1;
  int* seg_off = reinterpret_cast<int*>(w.v0);
  int* order = reinterpret_cast<int*>(w.k0);
  int* order2 = reinterpret_cast<int*>(w.k1);
  const bool cur = ctx->ins_count;
  if (cur) {
    // counted descent: the segments and their offsets exist (k_ins_descend<true>, k_ins_alloc_seg)
    k_ins_scatter_cur<<<g * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(n, nd, thread_num, m, w.leaf, order);
  } else {
    // leaves -> per-leaf buckets (no sort: the order between leaves is free)
    k_ins_resolve<<<g * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(n, nd, thread_num, w.pw, m, w.leaf, seg_leaf);
    k_seg_offsets<<<1, 1024, 0, s>>>(thread_num, m, seg_leaf, seg_off);
    k_ins_scatter<<<g * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(n, nd, thread_num, m, w.leaf, seg_off, order);
  }
  // ~one wave per leaf segment (the count stays on the device); plus the
  // recut's head when the recut follows in the same graph (ctx->rc_begin_wa)
  RcBeginArg rb;
  memset(&rb, 0, sizeof(rb));
  const bool has_rb = ctx->rc_begin_wa != nullptr;
  if (has_rb) {
    rb.wa = *ctx->rc_begin_wa;
    rb.st = ctx->st;
    rb.wpn = m.wpn;
    rb.win = (WinD*)ctx->ba.xs;
    rb.nper = (int*)((char*)ctx->ba.xs + sizeof(WinD));
    rb.slot_of = rb.nper + 32;  // (map_recut's dslot)
    rb.rc = w.rc;
    ctx->rc_begin_wa = nullptr;
    ctx->rc_begun = true;
  }
  auto push = cur ? (ctx->push_pipe ? k_push_window<true, true> : k_push_window<true, false>)
                  : (ctx->push_pipe ? k_push_window<false, true> : k_push_window<false, false>);
  push<<<gseg + (has_rb ? 1 : 0), 64 * kPushWaves, 0, s>>>(seg_leaf, seg_off, order, order2, mp, slot, m, w.pw, thread_num,
                                                            rb, has_rb ? 1 : 0);
  VG_HIP(hipGetLastError());
  return VG_OK;
}

// cut_voxel_multi (voxel_map.cpp:47-135) + pvec_update (point_utils.cpp:54-65).
// Asynchronous: every count stays on the device. A child-allocation overflow
// of k_ins_alloc sets kCntMisc; the insert tail and the recut kernels then skip
// and map_recut reports it (kNeedInsertReplay) for map_insert_replay.
int map_insert(vg_ctx* ctx, const MP& mp, int slot, int n, int epoch, int thread_num, const PushArg* push,
               const InsPre* pre, const int* nd) {
  DevMap& m = ctx->map;
  Work& w = ctx->wk;
  hipStream_t s = ctx->stream;
  if (n <= 0) {
    if (push) VG_TRY(state_push(ctx, push->ord, push->new_imu, push->rec));
    return VG_OK;
  }
  // device count: n is an upper bound, the kernels stride over the real one
  const int g = nd ? grid_for(n, kBlock, 2048) : grid_for(n);
  if (pre)
    k_ins_prep<true><<<g, kBlock, 0, s>>>(n, nullptr, nullptr, nullptr, nullptr, nullptr, mp, ctx->st, slot, m, w.pw,
                                          w.u0,
                                          nullptr, pre->pnt, pre->pose, pre->var_identity, nullptr, w.gran, w.ngran,
                                          nullptr);
  else {
    // the push record goes through host-mapped memory, so a replayed graph
    // picks up each scan's record (the host writes it before the launch)
    // (slot in_sel: a scan graph's ring position, whose per-scan numbers ride along)
    HostIn* hin = ctx->h_in + ctx->in_sel;
    HostIn* din = ctx->d_in + ctx->in_sel;
    if (push) hin->push = *push;
    k_ins_prep<false><<<g, kBlock, 0, s>>>(n, nd, ctx->ds.ox, ctx->ds.oy, ctx->ds.oz, ctx->ds.oi, mp, ctx->st, slot, m,
                                           w.pw,
                                           w.u0, push ? &din->push : nullptr, nullptr, nullptr, 0,
                                           nd ? ctx->ds.hflags : nullptr, w.gran, w.ngran,
                                           ctx->in_ph ? din->ph : nullptr);
  }
  const int ntile = (n + kRootTile - 1) / kRootTile;
  (void)epoch;
  if (ctx->roots_lb && ntile <= w.ngran) {  // one launch (decoupled look-back)
    k_ins_roots_lb<<<ntile, kBlock, 0, s>>>(n, nd, ntile, w.u0, mp, m, w.gran);
  } else {
    k_ins_flags<<<ntile, kBlock, 0, s>>>(n, nd, w.u0, m, w.v1, (int*)w.ac_cnt);
    k_ins_roots_alloc<<<ntile, kBlock, 0, s>>>(n, nd, ntile, w.u0, w.v1, (const int*)w.ac_cnt, mp, m);
  }
  if (sharded(ctx)) {  // the thread_num quirk counts distinct roots over all shards
    VG_TRY(shard_allreduce(ctx, m.counters + kCntTouched, m.counters + kCntGTouched, 1, 1, 1));
  }
  const int ins_cap = (ctx->dbg_ins_cap >= 0 && ctx->dbg_ins_cap < kInsAllocCap) ? ctx->dbg_ins_cap : kInsAllocCap;
  if (ctx->ins_count) {  // prep -> roots -> descend (+ counts) -> alloc || segment allocation -> scatter -> push
    k_ins_descend<true><<<g * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(n, nd, thread_num, w.pw, m, w.u0, w.leaf,
                                                                             w.list2, w.list1);
    k_ins_alloc_seg<<<1 + kSegAllocBlocks, 1024, 0, s>>>(thread_num, m, w.list2, ins_cap, w.list1,
                                                         reinterpret_cast<int2*>(w.v0));
  } else {
    k_ins_descend<false><<<g * (kBlock / kSpreadBlock), kSpreadBlock, 0, s>>>(n, nd, thread_num, w.pw, m, w.u0, w.leaf,
                                                                              w.list2, nullptr);
    k_ins_alloc<<<1, 1024, 0, s>>>(thread_num, m, w.list2, ins_cap);
  }
  return insert_tail(ctx, mp, slot, n, thread_num, nd);
}

// host-sized child allocation after a k_ins_alloc overflow, then the tail
int map_insert_replay(vg_ctx* ctx, const MP& mp, int slot, int n, int thread_num) {
  DevMap& m = ctx->map;
  hipStream_t s = ctx->stream;
  VG_TRY(read_counters(ctx));
  const int np = ctx->h_pinned[kCntCreate];
  VG_HIP(hipMemsetAsync(m.counters + kCntMisc, 0, sizeof(int), s));
  // (the counted descent's segments and request counts stand: its tail is the scatter and the push)
  if (!ctx->ins_count) VG_HIP(hipMemsetAsync(m.counters + kCntSeg, 0, sizeof(int), s));
  int created = 0;
  VG_TRY(alloc_children(ctx, ctx->wk.list2, np, nullptr, 0, false, &created));
  return insert_tail(ctx, mp, slot, n, thread_num);
}

// test hook (vgx_insert_segments): the last insert's segments while its work
// buffers still stand (right after vg_cut_voxel_multi) — per segment its key
// (a leaf id; with the counted descent a child request stays -2 - (parent * 8
// + octant)) and its length; info = {segments, roots touched, parents with
// child requests, abort flag}. Segments past cap are not written.
int map_insert_segments(vg_ctx* ctx, int* key, int* len, int cap, int* info) {
  DevMap& m = ctx->map;
  Work& w = ctx->wk;
  hipStream_t s = ctx->stream;
  int hc[kCntN];
  VG_HIP(hipMemcpyAsync(hc, m.counters, sizeof(hc), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  const int ns = hc[kCntSeg];
  info[0] = ns;
  info[1] = hc[kCntTouched];
  info[2] = hc[kCntCreate];
  info[3] = hc[kCntMisc];
  const int k = ns < cap ? ns : cap;
  if (k <= 0) return VG_OK;
  std::vector<int> off((size_t)2 * k + 2);
  VG_HIP(hipMemcpyAsync(key, w.list1, (size_t)k * sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(off.data(), w.v0, (ctx->ins_count ? (size_t)2 * k : (size_t)k + 1) * sizeof(int),
                        hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  for (int q = 0; q < k; q++) len[q] = ctx->ins_count ? off[2 * q + 1] : off[q + 1] - off[q];
  return VG_OK;
}

}  // namespace vg
