// map.hip — the device-resident adaptive voxel map: allocation, reset and the
// host helpers its stages share (insert.hip, recut.hip, margi.hip; the IEKF
// point loop that reads the map is iekf.hip).
//
// Layout in HBM (vg_internal.h DevMap): a root-voxel open-addressing hash
// (packed 63-bit key -> node id), a node pool of fixed records (NodeHdr 96 B for
// descent, PlaneRec 224 B for the gate, clusters/cov_add/eigen as separate
// arrays), SlideWindow clusters inline per node (W x 80 B), per-physical-slot
// window point arrays (body pnt, world var, owning leaf) and a point_fix arena.
// The reference's pointer-chasing recursion becomes level-synchronous
// worklists; per-leaf accumulation keeps the reference's point order by
// sorting (leaf, order) keys and walking each leaf's segment sequentially, so
// sums are deterministic and order-faithful.
#include <hipcub/hipcub.hpp>
#include "vg_map.h"

namespace vg {

// ------------------------------------------------------------------ alloc
int map_alloc(vg_ctx* ctx) {
  DevMap& m = ctx->map;
  const int W = ctx->cfg.win_size;
  m.W = W;
  m.cap_nodes = ctx->cap.max_nodes;
  m.cap_fix = ctx->cap.max_fix_points;
  m.hash_mask = (1 << ctx->cap.hash_log2) - 1;
  m.cap_wp = ctx->cap.max_points_per_scan;
  const size_t cn = m.cap_nodes, hs = (size_t)m.hash_mask + 1, cw = (size_t)m.cap_wp;
  auto ok = [&](void* p) { return p != nullptr; };
  bool good = true;
  good &= ok(m.hdr = ctx->arena.take<NodeHdr>(cn));
  good &= ok(m.pl = ctx->arena.take<PlaneRec>(cn));
  good &= ok(m.pcr_add = ctx->arena.take<Clu>(cn));
  good &= ok(m.pcr_fix = ctx->arena.take<Clu>(cn));
  good &= ok(m.cov_add = ctx->arena.take<double>(cn * kCovN));
  good &= ok(m.eig = ctx->arena.take<double>(cn * 12));
  good &= ok(m.jour = ctx->arena.take<double>(cn));
  good &= ok(m.dbox = ctx->arena.take<double>(cn * 6));
  good &= ok(m.pcrs = ctx->arena.take<Clu>(cn * W));
  good &= ok(m.nscr = ctx->arena.take<int>(cn * 4));
  good &= ok(m.pend = ctx->arena.take<unsigned long long>(cn));
  good &= ok(m.cfirst = ctx->arena.take<int>(cn * 8));
  good &= ok(m.hkey = ctx->arena.take<uint64_t>(hs));
  good &= ok(m.hval = ctx->arena.take<int>(hs));
  good &= ok(m.hfirst = ctx->arena.take<int>(hs));
  good &= ok(m.slide = ctx->arena.take<int>(cn));
  good &= ok(m.in_slide = ctx->arena.take<uint8_t>(cn));
  good &= ok(m.leaf_cnt = ctx->arena.take<int>(cn));
  good &= ok(m.leaf_seg = ctx->arena.take<int>(cn));
  good &= ok(m.creq_cnt = ctx->arena.take<int>(cn * 8));
  good &= ok(m.fix_pnt = ctx->arena.take<double>((size_t)m.cap_fix * 3));
  good &= ok(m.fix_var = ctx->arena.take<double>((size_t)m.cap_fix * 9));
  good &= ok(m.wp_pnt = ctx->arena.take<double>(cw * W * 3));
  good &= ok(m.wp_var = ctx->arena.take<double>(cw * W * 9));
  good &= ok(m.wp_leaf = ctx->arena.take<int>(cw * W));
  good &= ok(m.wp_int = ctx->arena.take<float>(cw * W));
  m.ord_stride = (int)(cw * (size_t)(ctx->cfg.max_layer + 1));
  good &= ok(m.wp_ord = ctx->arena.take<int>((size_t)m.ord_stride * W));
  good &= ok(m.lseg = ctx->arena.take<uint64_t>(cn * W));
  good &= ok(m.slot_epoch = ctx->arena.take<int>(kMaxWin));
  good &= ok(m.arena = ctx->arena.take<int>(kMaxWin));
  good &= ok(ctx->d_cmap = ctx->arena.take<float4>((cw + 2) / 3));
  good &= ok(ctx->d_cmap_n = ctx->arena.take<int>(4));
  good &= ok(m.counters = ctx->arena.take<int>(kCntN));
  good &= ok(m.stamp = ctx->arena.take<int>(cn));
  good &= ok(m.wpn = ctx->arena.take<int>(kMaxWin));
  Work& w = ctx->wk;
  w.cap = (int)(cw * (W + 1));
  good &= ok(w.k0 = ctx->arena.take<uint64_t>(w.cap));
  good &= ok(w.k1 = ctx->arena.take<uint64_t>(w.cap));
  good &= ok(w.v0 = ctx->arena.take<uint32_t>(w.cap));
  good &= ok(w.v1 = ctx->arena.take<uint32_t>(w.cap));
  good &= ok(w.u0 = ctx->arena.take<uint32_t>(w.cap));
  good &= ok(w.u1 = ctx->arena.take<uint32_t>(w.cap));
  good &= ok(w.ac_cnt = ctx->arena.take<uint32_t>(cn));
  good &= ok(w.ac_off = ctx->arena.take<uint32_t>(cn));
  good &= ok(w.cand = ctx->arena.take<int>(cn));
  good &= ok(w.list0 = ctx->arena.take<int>(cn));
  good &= ok(w.list1 = ctx->arena.take<int>(cn));
  good &= ok(w.list2 = ctx->arena.take<int>(cn));
  good &= ok(w.leaf = ctx->arena.take<int>(cw));
  good &= ok(w.pw = ctx->arena.take<double>(cw * 3));
  good &= ok(w.iekf_cache = ctx->arena.take<int>(cw));
  good &= ok(w.pk_leaf = ctx->arena.take<int>(cw));
  good &= ok(w.rc = ctx->arena.take<int>(128));
  good &= ok(w.cand_bits = ctx->arena.take<uint32_t>(ctx->cap.max_nodes / 32 + 1));
  good &= ok(w.plan = ctx->arena.take<int>(cn * 8));
  w.ngran = (int)(cw / 1024 + 64);
  good &= ok(w.gran = ctx->arena.take<unsigned long long>(w.ngran));
  good &= ok(w.sub_odd = ctx->arena.take<int>(cn));
  good &= ok(w.info_odd = ctx->arena.take<int>(w.cap));
  good &= ok(w.ev_odd = ctx->arena.take<uint64_t>(w.cap));
  w.nparts = 1024;
  good &= ok(w.partials = ctx->arena.take<double>((size_t)w.nparts * 40));
  if (!good) {
    ctx->err = "arena exhausted (map)";
    return VG_E_CAPACITY;
  }
  size_t b1 = 0, b2 = 0;
  VG_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, b1, w.k0, w.k1, w.cap, 0, 64, ctx->stream));
  VG_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, w.v0, w.v1, w.cap, ctx->stream));
  w.tmp_bytes = (b1 > b2 ? b1 : b2) + 256;
  w.tmp = ctx->arena.take<char>(w.tmp_bytes);
  w.tmp2 = ctx->arena.take<char>(w.tmp_bytes);  // the margi prefix sorts on the second stream
  if (!w.tmp || !w.tmp2) {
    ctx->err = "arena exhausted (sort workspace)";
    return VG_E_CAPACITY;
  }
  return VG_OK;
}

int map_reset(vg_ctx* ctx) {
  DevMap& m = ctx->map;
  hipStream_t s = ctx->stream;
  // Node records are handed out zeroed: the pool is cleared here (all of it
  // the first time, afterwards the ids handed out since), so no allocation on
  // the per-scan path writes a record it has not filled (ids are never reused
  // between resets)
  int used = m.cap_nodes;
  if (ctx->pool_zeroed) {
    VG_HIP(hipMemcpyAsync(ctx->h_pinned, m.counters, kCntN * sizeof(int), hipMemcpyDeviceToHost, s));
    VG_HIP(hipStreamSynchronize(s));
    used = ctx->h_pinned[kCntNodes] < m.cap_nodes ? ctx->h_pinned[kCntNodes] : m.cap_nodes;
  }
  if (used > 0) {
    const size_t u = (size_t)used;
    VG_HIP(hipMemsetAsync(m.pl, 0, u * sizeof(PlaneRec), s));
    VG_HIP(hipMemsetAsync(m.pcr_add, 0, u * sizeof(Clu), s));
    VG_HIP(hipMemsetAsync(m.pcr_fix, 0, u * sizeof(Clu), s));
    VG_HIP(hipMemsetAsync(m.cov_add, 0, u * kCovN * sizeof(double), s));
    VG_HIP(hipMemsetAsync(m.eig, 0, u * 12 * sizeof(double), s));
    VG_HIP(hipMemsetAsync(m.jour, 0, u * sizeof(double), s));
    VG_HIP(hipMemsetAsync(m.pcrs, 0, u * m.W * sizeof(Clu), s));
    VG_HIP(hipMemsetAsync(m.lseg, 0, u * m.W * sizeof(uint64_t), s));
  }
  ctx->pool_zeroed = true;
  const size_t hs = (size_t)m.hash_mask + 1;
  VG_HIP(hipMemsetAsync(m.hkey, 0xff, hs * sizeof(uint64_t), s));
  VG_HIP(hipMemsetAsync(m.hval, 0xff, hs * sizeof(int), s));
  VG_HIP(hipMemsetAsync(m.hfirst, 0x7f, hs * sizeof(int), s));
  VG_HIP(hipMemsetAsync(m.counters, 0, kCntN * sizeof(int), s));
  VG_HIP(hipMemsetAsync(m.stamp, 0, (size_t)m.cap_nodes * sizeof(int), s));
  VG_HIP(hipMemsetAsync(m.wpn, 0, kMaxWin * sizeof(int), s));
  VG_HIP(hipMemsetAsync(m.slot_epoch, 0, kMaxWin * sizeof(int), s));
  VG_HIP(hipMemsetAsync(m.arena, 0, kMaxWin * sizeof(int), s));
  VG_HIP(hipMemsetAsync(ctx->wk.cand_bits, 0, (ctx->cap.max_nodes / 32 + 1) * sizeof(uint32_t), s));
  VG_HIP(hipMemsetAsync(m.in_slide, 0, m.cap_nodes, s));
  VG_HIP(hipMemsetAsync(m.leaf_cnt, 0, (size_t)m.cap_nodes * sizeof(int), s));
  VG_HIP(hipMemsetAsync(m.cfirst, 0x7f, (size_t)m.cap_nodes * 8 * sizeof(int), s));
  VG_HIP(hipMemsetAsync(m.creq_cnt, 0, (size_t)m.cap_nodes * 8 * sizeof(int), s));
  VG_HIP(hipMemsetAsync(m.nscr, 0xff, (size_t)m.cap_nodes * 4 * sizeof(int), s));
  VG_HIP(hipStreamSynchronize(s));
  return ds_reset(ctx);  // the pipeline downsample's voxel table
}

// ------------------------------------------------------------------ shared host helpers (vg_map.h)
int read_counters(vg_ctx* ctx) {
  VG_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->map.counters, kCntN * sizeof(int), hipMemcpyDeviceToHost,
                        ctx->stream));
  VG_HIP(stream_wait(ctx));
  if (ctx->h_pinned[kCntErr]) {
    int e = ctx->h_pinned[kCntErr];
    ctx->err = std::string("device map error flags=") + std::to_string(e) +
               ((e & 4) ? " (node pool full)" : "") + ((e & 8) ? " (point_fix arena full)" : "") +
               ((e & 1) ? " (voxel key out of packed range)" : "") + ((e & 2) ? " (root hash full)" : "") +
               ((e & 16) ? " (subdivision event buffer full)" : "");
    return (e & 1) ? VG_E_RANGE : VG_E_CAPACITY;
  }
  return VG_OK;
}

static int excl_scan(vg_ctx* ctx, const uint32_t* in, uint32_t* out, int n) {
  size_t tb = ctx->wk.tmp_bytes;
  if (n <= 0) return VG_OK;
  VG_HIP(hipcub::DeviceScan::ExclusiveSum(ctx->wk.tmp, tb, in, out, n, ctx->stream));
  return VG_OK;
}
static int bits_for(long v) {
  int b = 1;
  while ((1L << b) <= v) b++;
  return b;
}

// sort a list of n (non-negative) node ids, ascending (deterministic creation
// order), over the id bits only; returns the buffer holding the result (`a` or
// the scratch w.u1 — k0/k1 may hold live events)
int sort_ids(vg_ctx* ctx, int* a, int n, int** result) {
  *result = a;
  if (n <= 1) return VG_OK;
  Work& w = ctx->wk;
  hipcub::DoubleBuffer<uint32_t> db(reinterpret_cast<uint32_t*>(a), w.u1);
  size_t tb = w.tmp_bytes;
  VG_HIP(hipcub::DeviceRadixSort::SortKeys(w.tmp, tb, db, n, 0, bits_for(ctx->map.cap_nodes), ctx->stream));
  *result = reinterpret_cast<int*>(db.Current());
  return VG_OK;
}
// in place
int sort_ids_inplace(vg_ctx* ctx, int* a, int n) {
  int* r = a;
  VG_TRY(sort_ids(ctx, a, n, &r));
  if (r != a) VG_HIP(hipMemcpyAsync(a, r, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
  return VG_OK;
}

// children for a sorted list of parents: ids = base + prefix(popcount(mask))
__global__ void __launch_bounds__(256) k_child_count(int np, const int* __restrict__ parents, DevMap m, uint32_t* __restrict__ cnt) {
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < np; q += gridDim.x * blockDim.x) {
    int p = parents[q];
    int c = 0;
    for (int o = 0; o < 8; o++) c += (m.cfirst[(size_t)p * 8 + o] == -5) ? 1 : 0;
    cnt[q] = (uint32_t)c;
  }
}

__global__ void __launch_bounds__(256) k_child_alloc(int np, const int* __restrict__ parents, const uint32_t* __restrict__ off, DevMap m,
                              int* __restrict__ next, int next_base) {
  const int base = m.counters[kCntNodes];
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < np; q += gridDim.x * blockDim.x)
    alloc_parent(m, parents[q], base + (int)off[q], next, next_base + (int)off[q]);
}

__global__ void __launch_bounds__(256) k_add_counter(int* counters, int idx, const uint32_t* __restrict__ flag,
                              const uint32_t* __restrict__ rank, int n) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && n > 0) counters[idx] += (int)(rank[n - 1] + flag[n - 1]);
}

// allocate children for the parents in plist (sorted), ids deterministic
int alloc_children(vg_ctx* ctx, int* plist, int np, int* next, int next_base, bool sorted, int* n_created) {
  Work& w = ctx->wk;
  hipStream_t s = ctx->stream;
  *n_created = 0;
  if (np <= 0) return VG_OK;
  if (!sorted) VG_TRY(sort_ids_inplace(ctx, plist, np));
  VG_TRY(read_counters(ctx));
  int first = ctx->h_pinned[kCntNodes];
  k_child_count<<<grid_for(np), kBlock, 0, s>>>(np, plist, ctx->map, w.ac_cnt);
  VG_TRY(excl_scan(ctx, w.ac_cnt, w.ac_off, np));
  k_child_alloc<<<grid_for(np), kBlock, 0, s>>>(np, plist, w.ac_off, ctx->map, next, next_base);
  k_add_counter<<<1, 64, 0, s>>>(ctx->map.counters, kCntNodes, w.ac_cnt, w.ac_off, np);
  VG_HIP(hipGetLastError());
  VG_TRY(read_counters(ctx));
  *n_created = ctx->h_pinned[kCntNodes] - first;
  return VG_OK;
}

}  // namespace vg
