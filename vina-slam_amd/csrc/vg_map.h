// vg_map.h — what more than one stage of the device-resident voxel map uses
// (map.hip, insert.hip, recut.hip, margi.hip): inline device helpers, shared
// constants and the host helpers defined in map.hip.
#pragma once
#include "vg_dev.h"

namespace vg {

// One-wave workgroups for the thread-per-item kernels whose work covers fewer
// workgroups than the chip has CUs (k_ins_descend / resolve / scatter over a
// scan's points, k_rc_visit, k_collect_level, the margi passes): their
// scattered record loads (64 cache lines per instruction) then spread over 4x
// the CUs' address units instead of queueing four waves deep on a quarter of
// them (k_margi_leaf 37.7 -> 32.9 us, k_rc_visit 15.0 -> 13.2 us)
constexpr int kSpreadBlock = 64;

// zero a freshly allocated node's records (the pool is zeroed lazily)
// children of parent p in octant order, ids id0, id0+1, ...; appended to next
__device__ __forceinline__ void alloc_parent(DevMap& m, int p, int id0, int* next, int next_pos) {
  NodeHdr& ph = m.hdr[p];
  int k = 0;
  for (int o = 0; o < 8; o++) {
    if (m.cfirst[(size_t)p * 8 + o] != -5) continue;
    const int id = id0 + k;
    k++;
    m.cfirst[(size_t)p * 8 + o] = 0x7f7f7f7f;
    if (id >= m.cap_nodes) {
      atomicOr(&m.counters[kCntErr], 4);
      continue;
    }
    int xyz[3] = {(o >> 2) & 1, (o >> 1) & 1, o & 1};
    double c[3];
    for (int j = 0; j < 3; j++) c[j] = ph.center[j] + (float)((2 * xyz[j] - 1) * ph.qlen);
    init_node(m.hdr[id], c, ph.qlen / 2, ph.layer + 1, p);
    dbox_child(m.dbox + (size_t)id * 6, m.dbox + (size_t)p * 6, ph.center, o);
    ph.child[o] = id;
    if (next) next[next_pos + k - 1] = id;
  }
  m.nscr[(size_t)p * 4 + 1] = -1;
}

// recut start: zero the level counts and the factor count; an insert whose
// child allocation overflowed (kCntMisc) blocks the whole recut (rc abort code
// kInsAbort) until map_insert_replay has run
constexpr int kInsAbort = 100;
__device__ __forceinline__ void recut_begin_block(DevMap& m, int* __restrict__ rc, int thread_num) {
  const int t = threadIdx.x;
  for (int i = t; i < kRcN; i += blockDim.x) rc[i] = 0;
  __syncthreads();
  if (t == 0) {
    m.counters[kCntFactors] = 0;
    m.counters[kCntGSlide] = m.counters[kCntSlide];  // all-reduced next in sharded mode
    if (m.counters[kCntMisc] != 0 && g_touched(m) >= thread_num) rc[kRcAbort] = kInsAbort;
  }
}

// host helpers of map.hip that insert.hip and recut.hip call; they stay out of
// the library's dynamic symbols, as they were while file-local
#pragma GCC visibility push(hidden)
// the map counters into ctx->h_pinned (synchronizes); the device error flags as a status
int read_counters(vg_ctx* ctx);
// sort a list of n (non-negative) node ids, ascending; *result: the buffer holding them
int sort_ids(vg_ctx* ctx, int* a, int n, int** result);
int sort_ids_inplace(vg_ctx* ctx, int* a, int n);
// allocate children for the parents in plist (sorted), ids deterministic
int alloc_children(vg_ctx* ctx, int* plist, int np, int* next, int next_base, bool sorted, int* n_created);
#pragma GCC visibility pop

}  // namespace vg
