// change.hip — the change layer's device side (vina_gpu.h "Change layer"):
// scan-vs-map evidence summed per map leaf and per cell of space over many
// scans. The layer lives beside a frozen map (ChangeDev, vg_internal.h); the
// map itself is only read, through the traversal of vg_ray.h.
//
// k_change_accum: one lane per point, 256-thread workgroups, no LDS. A point is
// classified by vg_diff.h's diff_point, the body k_scan_diff runs, so its
// record and the class counts have vg_scan_diff's bits; then the lane charges
// its leaf (one integer atomic on the class counter, an atomicMax on the
// leaf's epoch whose return tells the one lane per call that counts the scan)
// or, for an APPEARED point, its cell: a 64-bit atomicCAS claims the key slot
// by a linear probe bounded by the table size, then integer atomics on the
// slot. Nothing spins and nothing is floating point, so the layer's bits do not
// depend on the order the points, scans or callers arrive in. The atomics
// return nothing the lane waits for except the epoch's old value.
//
// The report is a flag / scan / compact pass over the node counters and over
// the cell table (k_change_count, k_change_scan, k_change_emit): a workgroup's
// selected items are counted, one workgroup turns the counts into offsets, and
// the records are built on the device at offset + rank, which keeps the index
// order: ascending node id for the leaves. The cells come out in slot order
// and are sorted by packed key on the host (change_report_dev).
#include <algorithm>

#include "vg_diff.h"

namespace vg {

struct ChangeQ {  // vg_change_query with the defaults applied
  int min_obs, min_scans, all, pad;
  double ratio;
};

// the cell of w: false when an index leaves the packed range
__device__ __forceinline__ bool chg_cell(const V3& w, double cell, unsigned long long& key, int q[3]) {
  bool ok = true;
  unsigned long long k[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double kf = floor(w[j] / cell);
    const bool in = kf > -(double)kKeyOff && kf < (double)kKeyOff;  // (a NaN fails both)
    ok = ok && in;
    double f = floor((w[j] - kf * cell) / cell * 65536.0);
    f = f >= 0.0 ? f : 0.0;
    f = f <= 65535.0 ? f : 65535.0;
    q[j] = in ? (int)f : 0;
    k[j] = in ? (unsigned long long)((long long)kf + kKeyOff) : 0ull;
  }
  key = (k[0] << 42) | (k[1] << 21) | k[2];
  return ok;
}

__global__ void __launch_bounds__(kRayBlock) k_change_accum(MP mp, DevMap m, ChangeDev L, const float* __restrict__ x,
                                                            const float* __restrict__ y, const float* __restrict__ z,
                                                            int stride, int n, Pose12 pose, DiffPrm prm, int epoch,
                                                            vg_diff_point* __restrict__ pp, double* __restrict__ absv,
                                                            int* __restrict__ sum) {
  const int i = blockIdx.x * kRayBlock + threadIdx.x;
  const bool valid = i < n;
  int cls = -1, rflags = 0;
  bool dropped = false, out_of_range = false;
  if (valid) {
    const size_t at = (size_t)i * (size_t)stride;
    const V3 pb = v3(x[at], y[at], z[at]);
    vg_diff_point dp;
    double av;
    V3 w;
    diff_point(mp, m, pb, pose, prm, dp, av, rflags, w);
    cls = dp.cls;
    if (pp) pp[i] = dp;
    absv[i] = av;
    // a classified point has a hit, and the layer is sized from the pool the hit's leaf lives in, so the
    // bound always holds; an APPEARED point it kept out would still be counted (out of range), which
    // keeps the totals' identity true by construction
    const int leaf = dp.leaf;
    const bool leaf_ok = leaf >= 0 && leaf < L.cap_nodes;
    if (cls == VG_DIFF_APPEARED && !leaf_ok) out_of_range = true;
    if (leaf_ok) {
      ChangeNode* N = &L.node[leaf];
      if (cls == VG_DIFF_APPEARED) {
        atomicAdd(&N->n_occluded, 1);
        unsigned long long key;
        int q[3];
        if (!chg_cell(w, L.cell_size, key, q)) {
          out_of_range = true;
        } else {
          uint32_t s = hash_slot(key, L.mask);
          int slot = -1;
          for (int probe = 0; probe <= L.mask; probe++) {
            const unsigned long long prev = atomicCAS(&L.ckey[s], (unsigned long long)kKeyEmpty, key);
            if (prev == kKeyEmpty || prev == key) {
              slot = (int)s;
              break;
            }
            s = (s + 1) & (uint32_t)L.mask;
          }
          if (slot < 0) {
            dropped = true;
          } else {
            ChangeCell* C = &L.cell[slot];
            atomicAdd(&C->n_appeared, 1);
#pragma unroll
            for (int j = 0; j < 3; j++)
              atomicAdd(reinterpret_cast<unsigned long long*>(&C->sum_q[j]), (unsigned long long)q[j]);
            if (atomicMax(&C->last_epoch, epoch) < epoch) atomicAdd(&C->n_scans, 1);
          }
        }
      } else if (cls == VG_DIFF_CONSISTENT || cls == VG_DIFF_VANISHED) {
        atomicAdd(cls == VG_DIFF_CONSISTENT ? &N->n_consistent : &N->n_vanished, 1);
        if (atomicMax(&N->last_epoch, epoch) < epoch) atomicAdd(&N->n_scans, 1);
      }
    }
  }
  diff_wave_counts(cls, valid, rflags, sum);
  const int lane = threadIdx.x & 63;
  const unsigned long long bd = __ballot(dropped), bo = __ballot(out_of_range);
  if (lane == 0 && bd) atomicAdd(reinterpret_cast<unsigned long long*>(&L.tot[kChgDropped]), (unsigned long long)__popcll(bd));
  if (lane == 0 && bo) atomicAdd(reinterpret_cast<unsigned long long*>(&L.tot[kChgOutOfRange]), (unsigned long long)__popcll(bo));
}

__global__ void __launch_bounds__(kBlock) k_change_clear(ChangeDev L) {
  const long step = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int* nodes = reinterpret_cast<int*>(L.node);
  const long nn = (long)L.cap_nodes * (long)(sizeof(ChangeNode) / sizeof(int));
  for (long i = t0; i < nn; i += step) nodes[i] = 0;
  const long ns = (long)L.mask + 1;
  for (long i = t0; i < ns; i += step) {
    L.ckey[i] = kKeyEmpty;
    ChangeCell c;
    c.sum_q[0] = c.sum_q[1] = c.sum_q[2] = 0;
    c.n_appeared = c.n_scans = c.last_epoch = c.pad = 0;
    L.cell[i] = c;
  }
  if (t0 < kChgTot) L.tot[t0] = 0;
}

// ---- the report. KIND 0: the nodes, 1: the cell table's slots
// used: the item holds evidence; meets: it meets its rule; returns whether the report takes it
template <int KIND>
__device__ __forceinline__ bool chg_select(const ChangeDev& L, const ChangeQ& q, int i, bool& used, bool& meets) {
  if (KIND == 0) {
    const ChangeNode N = L.node[i];
    used = (N.n_consistent | N.n_vanished | N.n_occluded) != 0;
    meets = N.n_vanished >= q.min_obs && N.n_scans >= q.min_scans &&
            (double)N.n_vanished >= q.ratio * (double)(N.n_vanished + N.n_consistent);
  } else {
    used = L.ckey[i] != kKeyEmpty;
    meets = false;
    if (used) {
      const ChangeCell& C = L.cell[i];
      meets = C.n_appeared >= q.min_obs && C.n_scans >= q.min_scans;
    }
  }
  meets = meets && used;
  return q.all ? used : meets;
}

// blk[b]: the items workgroup b's 256 indices select; agg[KIND]: the used items
template <int KIND>
__global__ void __launch_bounds__(kBlock) k_change_count(ChangeDev L, ChangeQ q, int n, int* __restrict__ blk,
                                                         unsigned long long* __restrict__ agg) {
  __shared__ int cnt[2];
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * kBlock + threadIdx.x;
  bool used = false, meets = false, sel = false;
  if (i < n) sel = chg_select<KIND>(L, q, i, used, meets);
  const unsigned long long bs = __ballot(sel), bu = __ballot(used);
  if ((threadIdx.x & 63) == 0) {
    if (bs) atomicAdd(&cnt[0], __popcll(bs));
    if (bu) atomicAdd(&cnt[1], __popcll(bu));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    blk[blockIdx.x] = cnt[0];
    if (cnt[1]) atomicAdd(&agg[KIND], (unsigned long long)cnt[1]);
  }
}

// one workgroup: blk[0 .. nb) to its exclusive prefix sums in place, the total to *total
__global__ void __launch_bounds__(kBlock) k_change_scan(int* __restrict__ blk, int nb, unsigned long long* __restrict__ total) {
  __shared__ int part[kBlock];
  const int t = threadIdx.x, per = (nb + kBlock - 1) / kBlock;
  const int lo = t * per < nb ? t * per : nb, hi = lo + per < nb ? lo + per : nb;
  int s = 0;
  for (int i = lo; i < hi; i++) s += blk[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = 0; k < kBlock; k++) {
      const int v = part[k];
      part[k] = run;
      run += v;
    }
    *total = (unsigned long long)run;
  }
  __syncthreads();
  int run = part[t];
  for (int i = lo; i < hi; i++) {
    const int v = blk[i];
    blk[i] = run;
    run += v;
  }
}

__device__ __forceinline__ void chg_leaf_record(const DevMap& m, const ChangeDev& L, int node, bool meets,
                                                vg_change_leaf& o) {
  const ChangeNode N = L.node[node];
  const NodeHdr& h = m.hdr[node];
  const PlaneRec& P = m.pl[node];
  o.node = node;
  o.layer = h.layer;
  o.n_consistent = N.n_consistent;
  o.n_vanished = N.n_vanished;
  o.n_occluded = N.n_occluded;
  o.n_scans = N.n_scans;
  o.flags = meets ? 1 : 0;
  o.pad = 0;
  // the fields vg_map_planes gives (markers.hip marker_eval): the normal normalised
  const double nn = sqrt(P.normal[0] * P.normal[0] + P.normal[1] * P.normal[1] + P.normal[2] * P.normal[2]);
  for (int j = 0; j < 3; j++) {
    o.voxel_center[j] = h.center[j];
    o.center[j] = P.center[j];
    o.normal[j] = nn > 0.0 ? P.normal[j] / nn : P.normal[j];
  }
  o.quater_length = (double)h.qlen;
}

__device__ __forceinline__ void chg_cell_record(const ChangeDev& L, int slot, bool meets, vg_change_cell& o) {
  const unsigned long long key = L.ckey[slot];
  const ChangeCell C = L.cell[slot];
  o.n_appeared = C.n_appeared;
  o.n_scans = C.n_scans;
  o.flags = meets ? 1 : 0;
  o.pad[0] = o.pad[1] = 0;
  for (int j = 0; j < 3; j++) {
    const long long k = (long long)((key >> (42 - 21 * j)) & ((1ull << 21) - 1)) - kKeyOff;
    o.key[j] = (int)k;
    const double na = (double)C.n_appeared;
    o.centroid[j] = L.cell_size * ((double)k + ((double)C.sum_q[j] + 0.5 * na) / (65536.0 * na));
  }
}

// the selected items' records at blk[workgroup] + the item's rank among the workgroup's selected; out holds cap
template <int KIND, typename Rec>
__global__ void __launch_bounds__(kBlock) k_change_emit(DevMap m, ChangeDev L, ChangeQ q, int n,
                                                        const int* __restrict__ blk, Rec* __restrict__ out, int cap) {
  __shared__ int wcnt[kBlock / 64];
  const int i = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool used = false, meets = false, sel = false;
  if (i < n) sel = chg_select<KIND>(L, q, i, used, meets);
  const unsigned long long b = __ballot(sel);
  if (lane == 0) wcnt[wave] = __popcll(b);
  __syncthreads();
  if (!sel) return;
  int pos = blk[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int k = 0; k < wave; k++) pos += wcnt[k];
  if (pos >= cap) return;
  Rec r;
  if constexpr (KIND == 0) {
    if (i >= m.cap_nodes) return;
    chg_leaf_record(m, L, i, meets, r);
  } else {
    chg_cell_record(L, i, meets, r);
  }
  out[pos] = r;
}

// ---- host side

int change_alloc(vg_ctx* ctx, ChangeLayer* L, int hash_log2) {
  static_assert(sizeof(ChangeNode) == 20 && sizeof(ChangeCell) == 40, "the layer's record sizes");
  static_assert(sizeof(vg_change_leaf) == 112 && sizeof(vg_change_cell) == 56 && sizeof(vg_change_totals) == 128,
                "the records' documented sizes");
  ChangeDev& d = L->d;
  d.cap_nodes = ctx->map.cap_nodes > 0 ? ctx->map.cap_nodes : 1;
  const size_t slots = (size_t)1 << hash_log2;
  d.mask = (int)(slots - 1);
  VG_HIP(L->node.reserve((size_t)d.cap_nodes));
  VG_HIP(L->ckey.reserve(slots));
  VG_HIP(L->cell.reserve(slots));
  VG_HIP(L->tot.reserve(8));  // kChgTot totals, then the report's scratch
  VG_HIP(L->blk.reserve((std::max((size_t)d.cap_nodes, slots) + kBlock - 1) / kBlock));
  d.node = L->node, d.ckey = L->ckey, d.cell = L->cell, d.tot = L->tot;
  return VG_OK;
}

int change_clear_dev(vg_ctx* ctx, ChangeLayer* L) {
  hipStream_t s = ctx->stream;
  const long n = std::max((long)L->d.cap_nodes * 5, (long)L->d.mask + 1);
  k_change_clear<<<grid_for(n, kBlock, 2048), kBlock, 0, s>>>(L->d);
  VG_HIP(hipGetLastError());
  VG_HIP(hipStreamSynchronize(s));
  return VG_OK;
}

int change_accum_dev(vg_ctx* ctx, ChangeLayer* L, const MP& mp, const float* x, const float* y, const float* z,
                     int stride, bool dev, int n, const double* pose12, int epoch, vg_diff_point* per_point,
                     vg_diff_summary* out) {
  memset(out, 0, sizeof(*out));
  if (n <= 0) return VG_OK;
  VG_TRY(ray_bufs(ctx));
  RayBufs& b = ctx->ray;
  hipStream_t s = ctx->stream;
  const DiffPrm q = diff_prm(&L->diff);
  Pose12 pose;
  for (int e = 0; e < 12; e++) pose.v[e] = pose12[e];
  vg_diff_point* d_pp = per_point ? reinterpret_cast<vg_diff_point*>(b.out.p) : nullptr;
  vg_diff_summary* d_sum = b.sum;
  if (!dev) {  // the host cloud, n x 3, into the staging vg_scan_diff uses
    float* d_xyz = reinterpret_cast<float*>(b.dir.p);
    VG_HIP(hipMemcpyAsync(d_xyz, x, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s));
    x = d_xyz, y = d_xyz + 1, z = d_xyz + 2;
  }
  VG_HIP(hipMemsetAsync(d_sum, 0, sizeof(vg_diff_summary), s));
  VG_HIP(b.t.begin(s));
  k_change_accum<<<(n + kRayBlock - 1) / kRayBlock, kRayBlock, 0, s>>>(mp, ctx->map, L->d, x, y, z, stride, n, pose, q,
                                                                      epoch, d_pp, b.org, reinterpret_cast<int*>(d_sum));
  diff_sum_launch(s, b.org, n, d_sum);
  VG_HIP(b.t.end(s));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(out, d_sum, sizeof(vg_diff_summary), hipMemcpyDeviceToHost, s));
  if (per_point) VG_HIP(hipMemcpyAsync(per_point, d_pp, (size_t)n * sizeof(vg_diff_point), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  return VG_OK;
}

// one flag / scan / compact pass: every selected record, in index order
template <int KIND, typename Rec>
static int change_pass(vg_ctx* ctx, ChangeLayer* L, const ChangeQ& q, int n, std::vector<Rec>& out) {
  hipStream_t s = ctx->stream;
  unsigned long long* agg = reinterpret_cast<unsigned long long*>(L->d.tot) + kChgTot;  // [0], [1]: used; [2]: selected
  const int nb = (n + kBlock - 1) / kBlock;
  out.clear();
  if (nb == 0) return VG_OK;
  if ((size_t)nb > L->blk.cap) {
    ctx->err = "vg_change_report: more items than the layer's scratch was sized for";
    return VG_E_STATE;
  }
  int* d_blk = L->blk;
  k_change_count<KIND><<<nb, kBlock, 0, s>>>(L->d, q, n, d_blk, agg);
  VG_HIP(hipGetLastError());
  k_change_scan<<<1, kBlock, 0, s>>>(d_blk, nb, agg + 2);
  VG_HIP(hipGetLastError());
  unsigned long long total = 0;
  VG_HIP(hipMemcpyAsync(&total, agg + 2, sizeof(total), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  if (total == 0) return VG_OK;
  const size_t bytes = (size_t)total * sizeof(Rec);
  // the record staging, kept in the layer and grown geometrically
  if (bytes > L->out.cap) VG_HIP(L->out.reserve(std::max(bytes, (size_t)1 << 16) * 2));
  Rec* d_out = reinterpret_cast<Rec*>(L->out.p);
  k_change_emit<KIND, Rec><<<nb, kBlock, 0, s>>>(ctx->map, L->d, q, n, d_blk, d_out, (int)total);
  VG_HIP(hipGetLastError());
  out.resize((size_t)total);
  VG_HIP(hipMemcpyAsync(out.data(), d_out, bytes, hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  return VG_OK;
}

int change_report_dev(vg_ctx* ctx, ChangeLayer* L, const vg_change_query& query, std::vector<vg_change_leaf>& leaves,
                      std::vector<vg_change_cell>& cells, long long* tot4) {
  ChangeQ q;
  q.min_obs = query.min_obs > 0 ? query.min_obs : 5;
  q.min_scans = query.min_scans > 0 ? query.min_scans : 2;
  q.ratio = query.vanished_ratio > 0.0 ? query.vanished_ratio : 0.8;
  q.all = query.flags & 1;
  q.pad = 0;
  hipStream_t s = ctx->stream;
  const int slots = L->d.mask + 1;
  // a leaf's record reads the map the caller's context reads: the owner's pool, whichever context asks
  const int n_nodes = std::min(L->d.cap_nodes, ctx->map.cap_nodes);
  VG_HIP(hipMemsetAsync(L->d.tot + kChgTot, 0, 3 * sizeof(long long), s));
  VG_TRY((change_pass<0, vg_change_leaf>(ctx, L, q, n_nodes, leaves)));
  VG_TRY((change_pass<1, vg_change_cell>(ctx, L, q, slots, cells)));
  VG_HIP(hipMemcpy(tot4, L->d.tot, 4 * sizeof(long long), hipMemcpyDeviceToHost));
  auto packed = [](const vg_change_cell& c) {
    return ((uint64_t)(c.key[0] + kKeyOff) << 42) | ((uint64_t)(c.key[1] + kKeyOff) << 21) | (uint64_t)(c.key[2] + kKeyOff);
  };
  std::sort(cells.begin(), cells.end(),
            [&](const vg_change_cell& a, const vg_change_cell& b) { return packed(a) < packed(b); });
  return VG_OK;
}

}  // namespace vg
