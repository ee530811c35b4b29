// map_dump.cpp — vgx_map_nodes (test hook): the device map
// node for node, in the record of the oracle's orc_map_nodes
// (oracle/vina_oracle.h), for a field-by-field comparison of the two maps.
// No kernel: the live prefix of the pool arrays is copied to the host after
// the outstanding work has completed (as vg_map_planes does) and the records
// are assembled here. Nothing on the device is written.
#include <cstring>

#include "vg_host.h"

namespace vg {
namespace {

struct Dump {
  int n = 0;
  std::vector<double> rec, fixp, winp;
  std::vector<long long> fix_off, win_off;
};

template <class T>
int pull(vg_ctx* ctx, std::vector<T>& h, const T* d, size_t n) {
  h.resize(n);
  if (n > 0) VG_HIP(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return VG_OK;
}
inline long long key_axis(uint64_t key, int sh) { return (long long)((key >> sh) & ((1ull << 21) - 1)) - kKeyOff; }
inline void put_clu(double* q, const Clu& c) {
  q[0] = c.N;
  for (int i = 0; i < 3; i++) q[1 + i] = c.v[i];
  for (int i = 0; i < 6; i++) q[4 + i] = c.P[i];
}

int build(vg_ctx* ctx, Dump& D) {
  const DevMap& m = ctx->map;
  HostPipe* P = hp(ctx);
  const int W = m.W, R = kNodeRec + kNodeSlot * W;
  std::vector<int> hc;
  VG_TRY(pull(ctx, hc, m.counters, (size_t)kCntN));
  const size_t n = (size_t)std::max(0, std::min(hc[kCntNodes], m.cap_nodes));
  const size_t nfix = (size_t)std::max(0, std::min(hc[kCntFix], m.cap_fix));
  std::vector<NodeHdr> hdr;
  std::vector<PlaneRec> pl;
  std::vector<Clu> add, fix, pcrs;
  std::vector<double> cov, eig, jour, fpnt, fvar;
  std::vector<uint64_t> lseg, hkey;
  std::vector<int> hval, epoch, wpn, ord;
  VG_TRY(pull(ctx, hdr, m.hdr, n));
  VG_TRY(pull(ctx, pl, m.pl, n));
  VG_TRY(pull(ctx, add, m.pcr_add, n));
  VG_TRY(pull(ctx, fix, m.pcr_fix, n));
  VG_TRY(pull(ctx, pcrs, m.pcrs, n * W));
  VG_TRY(pull(ctx, cov, m.cov_add, n * kCovN));
  VG_TRY(pull(ctx, eig, m.eig, n * 12));
  VG_TRY(pull(ctx, jour, m.jour, n));
  VG_TRY(pull(ctx, lseg, m.lseg, n * W));
  VG_TRY(pull(ctx, hkey, m.hkey, (size_t)m.hash_mask + 1));
  VG_TRY(pull(ctx, hval, m.hval, (size_t)m.hash_mask + 1));
  VG_TRY(pull(ctx, epoch, m.slot_epoch, (size_t)kMaxWin));
  VG_TRY(pull(ctx, wpn, m.wpn, (size_t)W));
  VG_TRY(pull(ctx, ord, m.wp_ord, (size_t)W * m.ord_stride));
  VG_TRY(pull(ctx, fpnt, m.fix_pnt, nfix * 3));
  VG_TRY(pull(ctx, fvar, m.fix_var, nfix * 9));
  // the window points of each physical slot: the prefix its last insert wrote
  std::vector<std::vector<double>> wpnt(W), wvar(W);
  for (int s = 0; s < W; s++) {
    const size_t k = (size_t)std::max(0, std::min(wpn[s], m.cap_wp));
    VG_TRY(pull(ctx, wpnt[s], m.wp_pnt + (size_t)s * m.cap_wp * 3, k * 3));
    VG_TRY(pull(ctx, wvar[s], m.wp_var + (size_t)s * m.cap_wp * 9, k * 9));
  }
  // A leaf's run in a slot is its sw->points[slot] when the run is of the
  // slot's current epoch AND the slot holds a scan of the window. The second
  // condition is the device's own representation of margi's
  // sw->points[mp[0]].clear() (octree.cpp:474-478): margi zeroes the slot's
  // cluster but leaves the lseg words, which stay of the current epoch until
  // the next insert into that slot bumps it; every reader of a run
  // (recut.hip k_rc_*: lanes <= win_count; margi.hip: mp[0] of a full window)
  // takes ring positions below win_count only. Without it the vacated slot of
  // every margi'd leaf would show its marginalised points as still listed.
  // The slot's cluster is dumped unmasked, so a slot outside the window that
  // still held points would differ from the oracle's zeros there.
  std::vector<char> in_win(W, 0);
  for (int i = 0; i < P->win_count && i < W && i < (int)P->mp.size(); i++)
    if (P->mp[i] >= 0 && P->mp[i] < W) in_win[P->mp[i]] = 1;

  D = Dump();
  D.fix_off.push_back(0);
  D.win_off.push_back(0);
  auto bad = [&](const std::string& what) {
    ctx->err = "vgx_map_nodes: " + what;
    return VG_E_STATE;
  };
  struct Item {
    int node, depth;
    int path[8];
  };
  std::vector<Item> stack;
  for (size_t s = 0; s < hkey.size(); s++) {
    if (hkey[s] == kKeyEmpty) continue;
    const int root = hval[s];
    if (root < 0 || (size_t)root >= n) continue;
    if (hdr[root].parent >= 0) return bad("hashed node " + std::to_string(root) + " has a parent");
    Item it0 = Item();
    it0.node = root;
    it0.depth = 0;
    stack.push_back(it0);
    while (!stack.empty()) {
      const Item it = stack.back();
      stack.pop_back();
      const int id = it.node;
      const NodeHdr& h = hdr[id];
      D.rec.resize(D.rec.size() + R, 0.0);
      double* r = D.rec.data() + D.rec.size() - R;
      r[0] = (double)key_axis(hkey[s], 42);
      r[1] = (double)key_axis(hkey[s], 21);
      r[2] = (double)key_axis(hkey[s], 0);
      r[3] = it.depth;
      for (int i = 0; i < 8; i++) r[4 + i] = i < it.depth ? it.path[i] : -1;
      int mask = 0;
      for (int o = 0; o < 8; o++)
        if (h.child[o] >= 0) mask |= 1 << o;
      r[12] = h.layer;
      r[13] = h.octo;
      r[14] = h.isexist;
      r[15] = h.is_plane;
      r[16] = mask;
      r[17] = h.last_num;
      r[18] = h.opt_state;
      r[19] = h.has_sw;
      for (int i = 0; i < 3; i++) r[20 + i] = h.center[i];
      r[23] = h.qlen;
      r[24] = it.depth == 0 ? jour[id] : 0.0;
      put_clu(r + 25, fix[id]);
      put_clu(r + 35, add[id]);
      memcpy(r + 45, &cov[(size_t)id * kCovN], kCovN * sizeof(double));
      for (int i = 0; i < 3; i++) r[90 + i] = pl[id].center[i];
      for (int i = 0; i < 3; i++) r[93 + i] = pl[id].normal[i];
      memcpy(r + 96, pl[id].var, 21 * sizeof(double));
      r[117] = pl[id].radius;
      memcpy(r + 118, &eig[(size_t)id * 12], 12 * sizeof(double));
      const int fc = h.fix_cnt > 0 ? h.fix_cnt : 0;
      if (fc > 0 && (h.fix_off < 0 || (size_t)h.fix_off + fc > nfix))
        return bad("point_fix block of node " + std::to_string(id) + " outside the arena");
      r[130] = fc;
      for (int j = 0; j < fc; j++) {
        const size_t f = (size_t)h.fix_off + j;
        D.fixp.insert(D.fixp.end(), &fpnt[f * 3], &fpnt[f * 3] + 3);
        D.fixp.insert(D.fixp.end(), &fvar[f * 9], &fvar[f * 9] + 9);
      }
      D.fix_off.push_back((long long)D.fixp.size() / 12);
      for (int sl = 0; sl < W; sl++) {
        double* q = r + kNodeRec + kNodeSlot * sl;
        if (h.has_sw) {
          put_clu(q + 1, pcrs[(size_t)id * W + sl]);
          const uint64_t v = lseg[(size_t)id * W + sl];
          const int st = (int)(v & 0xffffff), len = (int)((v >> 24) & 0x1fffff);
          if (in_win[sl] && len > 0 && (int)(v >> 45) == (epoch[sl] & 0x7ffff)) {
            if (st + len > m.ord_stride) return bad("run of node " + std::to_string(id) + " outside wp_ord");
            q[0] = len;
            for (int j = 0; j < len; j++) {
              const int i = ord[(size_t)sl * m.ord_stride + st + j];
              if (i < 0 || (size_t)i * 3 >= wpnt[sl].size())
                return bad("run of node " + std::to_string(id) + " names a point outside its slot");
              D.winp.insert(D.winp.end(), &wpnt[sl][(size_t)i * 3], &wpnt[sl][(size_t)i * 3] + 3);
              D.winp.insert(D.winp.end(), &wvar[sl][(size_t)i * 9], &wvar[sl][(size_t)i * 9] + 9);
            }
          }
        }
        D.win_off.push_back((long long)D.winp.size() / 12);
      }
      D.n++;
      for (int o = 7; o >= 0; o--) {
        const int c = h.child[o];
        if (c < 0) continue;
        if ((size_t)c >= n || hdr[c].parent != id || it.depth >= 8)
          return bad("child " + std::to_string(c) + " of node " + std::to_string(id) + " is not linked back");
        Item nx = it;
        nx.node = c;
        nx.path[it.depth] = o;
        nx.depth = it.depth + 1;
        stack.push_back(nx);
      }
    }
  }
  return VG_OK;
}

}  // namespace

int host_map_nodes(vg_ctx* ctx, double* rec, int cap, double* fixp, long long* fix_off, double* winp,
                   long long* win_off, long long* info) {
  if (ctx->view_of || ctx->views > 0) {
    ctx->err = "vgx_map_nodes: the map is shared (vg_map_attach)";
    return VG_E_STATE;
  }
  VG_TRY(refuse_fleet(ctx, "vgx_map_nodes"));
  if (ctx->shard.world > 1) {
    ctx->err = "vgx_map_nodes: the context is sharded (world > 1)";
    return VG_E_STATE;
  }
  VG_TRY(host_quiesce(ctx));
  Dump D;  // made anew by every call: nothing is kept between the count call and the data call
  VG_TRY(build(ctx, D));
  HostPipe* P = hp(ctx);
  const int W = ctx->map.W;
  const bool fits = rec && cap == D.n && info[1] == D.fix_off.back() && info[2] == D.win_off.back();
  info[0] = D.n;
  info[1] = D.fix_off.back();
  info[2] = D.win_off.back();
  info[3] = P->win_count;
  info[4] = W;
  for (int i = 0; i < W; i++) info[5 + i] = i < (int)P->mp.size() ? P->mp[i] : -1;
  if (!rec) return VG_OK;
  if (!fits) {
    ctx->err = "vgx_map_nodes: the map is not the one the count call saw (nodes / points differ)";
    return VG_E_ARG;
  }
  if (!D.rec.empty()) memcpy(rec, D.rec.data(), D.rec.size() * sizeof(double));
  if (!D.fixp.empty()) memcpy(fixp, D.fixp.data(), D.fixp.size() * sizeof(double));
  if (!D.winp.empty()) memcpy(winp, D.winp.data(), D.winp.size() * sizeof(double));
  memcpy(fix_off, D.fix_off.data(), D.fix_off.size() * sizeof(long long));
  memcpy(win_off, D.win_off.data(), D.win_off.size() * sizeof(long long));
  return VG_OK;
}

}  // namespace vg
