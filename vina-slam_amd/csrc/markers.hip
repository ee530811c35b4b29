// markers.hip — the map's plane / normal markers, collected on the device.
//
// The reference publishes /voxel_plane and /voxel_normal after every
// steady-state multi_recut (local_mapping.cpp:455-470) by walking
// surf_map_slide with OctoTree::collect_plane_markers / collect_normal_markers
// (octree.cpp:758-949). Here one kernel walks the same subtrees, applies the
// same per-node rule to the publication flags in NodeHdr::mk and appends one
// record per event (vg_plane_marker, include/vina_gpu.h); a second kernel
// snapshots the map in the same record type (vg_map_planes). Nothing here
// runs unless vg_set_publish bit 1 is set or vg_map_planes is called.
#include "vg_map.h"

namespace vg {

constexpr int kMkDepth = 8;     // layers the walks descend (max_layer < kMkDepth, checked by the host)
constexpr int kMkGrid = 64;     // the collection's fixed grid (x kBlock lanes, one slide root per lane and round)
constexpr double kMkAlpha = 0.8, kMkMaxTrace = 0.25, kMkPow = 0.2;  // the collectors' defaults (octree.hpp)

// voxel_id_from_center (octree.cpp:11-21): the hash in wrap-around int64 arithmetic
__device__ __forceinline__ int32_t marker_id(const double c[3], int layer) {
  const uint64_t ix = (uint64_t)llround(c[0] * 1000.0);
  const uint64_t iy = (uint64_t)llround(c[1] * 1000.0);
  const uint64_t iz = (uint64_t)llround(c[2] * 1000.0);
  uint64_t h = (ix * 73856093ull) ^ (iy * 19349663ull) ^ (iz * 83492791ull) ^ ((uint64_t)(int64_t)layer * 2654435761ull);
  if ((int64_t)h < 0) h = 0ull - h;
  return (int32_t)(h & 0x7fffffffull);
}

// The colour ramp of map_jet (octree.cpp:23-63) as one expression per channel
// over its five segments [0, b0) [b0, b1) [b1, b2) [b2, b3) [b3, 1]: blue rises
// from 0.504, holds, falls; green rises, holds, falls; red rises, holds, falls
// to 0.504. Each channel keeps the ramp's fp64 arithmetic, so the truncated
// bytes are the reference's.
__device__ __forceinline__ void marker_jet(double v, int& r, int& g, int& b) {
  constexpr double b0 = 0.1242, b1 = 0.3747, b2 = 0.6253, b3 = 0.8758, lo = 0.504;
  v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
  const int seg = (v < b0) ? 0 : (v < b1) ? 1 : (v < b2) ? 2 : (v < b3) ? 3 : 4;
  const double red = seg < 2 ? 0.0 : seg == 2 ? (v - b1) * (1.0 / (b2 - b1))
                   : seg == 3 ? 1.0 : 1.0 - (v - b3) * ((1.0 - lo) / (1.0 - b3));
  const double green = seg == 1 ? (v - b0) * (1.0 / (b1 - b0)) : seg == 2 ? 1.0
                     : seg == 3 ? (b3 - v) * (1.0 / (b3 - b2)) : 0.0;
  const double blue = seg == 0 ? lo + ((1.0 - lo) / b0) * v : seg == 1 ? 1.0
                    : seg == 2 ? (b2 - v) * (1.0 / (b2 - b1)) : 0.0;
  r = (int)(uint8_t)(255 * red);
  g = (int)(uint8_t)(255 * green);
  b = (int)(uint8_t)(255 * blue);
}

// The marker math of octree.cpp:11-63, 787-824, 900-917 on one node's values:
// every field of the record but action and flags. normal may be unnormalised
// (a zero normal stays zero: a node without a plane).
__device__ void marker_eval(const double vc[3], int layer, double qlen, const double center[3],
                            const double normal[3], double trace, const double eig[3], vg_plane_marker& o) {
  for (int j = 0; j < 3; j++) {
    o.voxel_center[j] = vc[j];
    o.center[j] = center[j];
    o.eig[j] = eig[j];
  }
  o.quater_length = qlen;
  o.trace = trace;
  o.layer = layer;
  o.id = marker_id(vc, layer);
  // colour: trace clamped at max_trace, scaled, pow, map_jet, bytes / 255.0f
  double t = trace;
  if (!(t > 0.0)) t = 0.0;  // (a node without a plane: a stale or empty record must not reach pow as a negative or NaN)
  if (t >= kMkMaxTrace) t = kMkMaxTrace;
  t = t * (1.0 / kMkMaxTrace);
  t = pow(t, kMkPow);
  int r, g, b;
  marker_jet(t, r, g, b);
  o.rgba[0] = r / 255.0f;
  o.rgba[1] = g / 255.0f;
  o.rgba[2] = b / 255.0f;
  o.rgba[3] = (float)kMkAlpha;
  // plane.normal.normalized()
  const double nn = sqrt(normal[0] * normal[0] + normal[1] * normal[1] + normal[2] * normal[2]);
  double n[3];
  for (int j = 0; j < 3; j++) n[j] = nn > 0.0 ? normal[j] / nn : normal[j];
  for (int j = 0; j < 3; j++) o.normal[j] = n[j];
  // Quaterniond::FromTwoVectors(UnitZ, n): c = z . n, axis = z x n = (-ny, nx, 0)
  const double c = n[2];
  if (c >= -1.0 + 1e-12) {
    const double s = sqrt(2.0 * (1.0 + c));
    o.quat[0] = -n[1] / s;
    o.quat[1] = n[0] / s;
    o.quat[2] = 0.0;
    o.quat[3] = s / 2.0;
  } else {
    // n ~ -z, where Eigen's SVD picks an arbitrary perpendicular axis: the half
    // turn about x (z -> -z) followed by the well-conditioned rotation -z -> n
    const double s = sqrt(2.0 * (1.0 - c));
    o.quat[0] = s / 2.0;
    o.quat[1] = 0.0;
    o.quat[2] = n[0] / s;
    o.quat[3] = -n[1] / s;
  }
  const double ev0 = eig[0] > 0.0 ? eig[0] : 0.0, ev1 = eig[1] > 0.0 ? eig[1] : 0.0, ev2 = eig[2] > 0.0 ? eig[2] : 0.0;
  o.plane_scale[0] = 3.0 * sqrt(ev2);
  o.plane_scale[1] = 3.0 * sqrt(ev1);
  o.plane_scale[2] = 2.0 * sqrt(ev0);
  const double length = 2.0 * qlen;
  for (int j = 0; j < 3; j++) o.tip[j] = center[j] + n[j] * length;
  o.normal_scale[0] = 0.1 * length;
  o.normal_scale[1] = 0.2 * length;
  o.normal_scale[2] = 0.0;
}

__device__ __forceinline__ void marker_zero(vg_plane_marker& o) {
  double* d = (double*)&o;
  for (int j = 0; j < (int)(sizeof(vg_plane_marker) / sizeof(double)); j++) d[j] = 0.0;
}

// one node's record: the marker fields when it holds a plane (`full`), else
// the identifying fields alone
__device__ void marker_of_node(const DevMap& m, int node, int action, int flags, bool full, vg_plane_marker& o) {
  const NodeHdr& h = m.hdr[node];
  marker_zero(o);
  if (full) {
    const PlaneRec& P = m.pl[node];
    const double trace = (P.var[sym_idx(6, 0, 0)] + P.var[sym_idx(6, 1, 1)]) + P.var[sym_idx(6, 2, 2)];
    marker_eval(h.center, h.layer, (double)h.qlen, P.center, P.normal, trace, &m.eig[(size_t)node * 12], o);
  } else {
    for (int j = 0; j < 3; j++) o.voxel_center[j] = h.center[j];
    o.quater_length = (double)h.qlen;
    o.layer = h.layer;
    o.id = marker_id(h.center, h.layer);
  }
  o.action = action;
  o.flags = flags;
}

__device__ __forceinline__ int marker_flags(const NodeHdr& h, int in_slide) {
  return (h.is_plane ? 1 : 0) | (h.octo ? 2 : 0) | (in_slide ? 4 : 0) | ((h.mk & kMkUpdated) ? 8 : 0) |
         ((h.mk & kMkPublished) ? 16 : 0);
}

// Depth-first walk of one subtree per lane, one node per lane and round, so
// the whole wave meets at the wave-aggregated appends: next node of the lane's
// walk, or -1 when it is over. sn / so: per level the node and its next octant.
struct MkWalk {
  int sn[kMkDepth];
  int so[kMkDepth];
  int d, root;
};
__device__ __forceinline__ void walk_begin(MkWalk& w, int root) {
  w.d = -1;
  w.root = root;
}
__device__ __forceinline__ int walk_next(MkWalk& w, const DevMap& m) {
  if (w.root >= 0) {
    const int r = w.root;
    w.root = -1;
    return r;
  }
  while (w.d >= 0) {
    const NodeHdr& h = m.hdr[w.sn[w.d]];
    int o = w.so[w.d];
    while (o < 8 && h.child[o] < 0) o++;
    if (o < 8) {
      w.so[w.d] = o + 1;
      return h.child[o];
    }
    w.d--;
  }
  return -1;
}
// descend into `node` next (an internal node above max_layer)
__device__ __forceinline__ void walk_push(MkWalk& w, int node) {
  if (w.d + 1 >= kMkDepth) return;
  w.d++;
  w.sn[w.d] = node;
  w.so[w.d] = 0;
}

// The collection (local_mapping.cpp:455-470): every node of the surf_map_slide
// subtrees, the rule of octree.cpp:761-850 on its flags. The slide count is
// read on the device (fixed grid, grid-stride over the roots). A subtree is
// walked by one lane and a node belongs to one subtree, so the flags need no
// atomics and no order between workgroups. An event's slot is reserved (one
// atomic per wave) before its node's flags change: an event past the buffer
// leaves them as they are and comes out on a later scan; cnt[0] counts the
// reservations, so the events past `cap` are the deferred ones.
__global__ void __launch_bounds__(kBlock) k_mk_collect(DevMap m, int max_layer, vg_plane_marker* __restrict__ out,
                                                       int cap, int* __restrict__ cnt) {
  const int ns = m.counters[kCntSlide];
  for (int base = blockIdx.x * blockDim.x; base < ns; base += gridDim.x * blockDim.x) {
    const int q = base + threadIdx.x;
    MkWalk w;
    walk_begin(w, q < ns ? m.slide[q] : -1);
    for (;;) {
      const int node = walk_next(w, m);
      if (!__any(node >= 0)) break;
      int action = -1;
      if (node >= 0) {
        NodeHdr& h = m.hdr[node];
        if (h.layer <= max_layer) {
          if (h.octo == 0) {
            if (!h.is_plane && (h.mk & kMkPublished)) action = 2;
            else if (h.is_plane && (h.mk & kMkUpdated)) action = 0;
          } else {
            if (h.mk & kMkPublished) action = 2;
            if (h.layer < max_layer) walk_push(w, node);
          }
        }
      }
      const int slot = wave_append(cnt, action >= 0 ? 1 : 0);
      if (action >= 0 && slot < cap) {
        NodeHdr& h = m.hdr[node];
        vg_plane_marker rec;
        marker_of_node(m, node, action, marker_flags(h, 1), action == 0, rec);
        out[slot] = rec;
        h.mk = (int8_t)(action == 0 ? kMkPublished : 0);
      }
    }
  }
}

// vg_map_planes: the subtrees of the hashed roots (sel bit 0: those in
// surf_map_slide only), plane leaves (sel bit 1: every node with layer <=
// max_layer); out == nullptr counts only
__global__ void __launch_bounds__(kBlock) k_mk_snapshot(DevMap m, int n_nodes, int max_layer, int sel,
                                                        vg_plane_marker* __restrict__ out, int cap,
                                                        int* __restrict__ cnt) {
  const int hs = m.hash_mask + 1;
  for (int base = blockIdx.x * blockDim.x; base < hs; base += gridDim.x * blockDim.x) {
    const int s = base + threadIdx.x;
    int root = -1;
    if (s < hs && m.hkey[s] != kKeyEmpty) {
      const int r = m.hval[s];
      if (r >= 0 && r < n_nodes && (!(sel & 1) || m.in_slide[r])) root = r;
    }
    const int slide = root >= 0 ? (int)m.in_slide[root] : 0;
    MkWalk w;
    walk_begin(w, root);
    for (;;) {
      const int node = walk_next(w, m);
      if (!__any(node >= 0)) break;
      int take = 0;
      if (node >= 0) {
        const NodeHdr& h = m.hdr[node];
        if (h.layer <= max_layer) {
          take = (sel & 2) ? 1 : (h.octo == 0 && h.is_plane ? 1 : 0);
          if (h.octo != 0 && h.layer < max_layer) walk_push(w, node);
        }
      }
      const int slot = wave_append(cnt, take);
      if (take && out && slot < cap) {
        const NodeHdr& h = m.hdr[node];
        vg_plane_marker rec;
        marker_of_node(m, node, 0, marker_flags(h, slide), true, rec);
        out[slot] = rec;
      }
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_mk_clear(DevMap m, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) m.hdr[i].mk = 0;
}

// vgx_marker_eval: marker_eval on caller-supplied inputs, 15 doubles per item
// (voxel_center 3, layer, qlen, center 3, normal 3, trace, eig 3)
constexpr int kMkEvalIn = 15;
__global__ void __launch_bounds__(kBlock) k_mk_eval(const double* __restrict__ in, int n, vg_plane_marker* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* a = in + (size_t)i * kMkEvalIn;
  vg_plane_marker rec;
  marker_zero(rec);
  marker_eval(a, (int)a[3], a[4], a + 5, a + 8, a[11], a + 12, rec);
  out[i] = rec;
}

static int used_nodes(vg_ctx* ctx, int* n) {
  int c = 0;
  VG_HIP(hipMemcpy(&c, ctx->map.counters + kCntNodes, sizeof(int), hipMemcpyDeviceToHost));
  *n = c < ctx->map.cap_nodes ? (c < 0 ? 0 : c) : ctx->map.cap_nodes;
  return VG_OK;
}

// the caller has completed the outstanding work (vg_set_publish)
int markers_enable(vg_ctx* ctx, bool on) {
  if (on && ctx->cfg.max_layer >= kMkDepth) {
    ctx->err = "vg_set_publish: markers need max_layer < " + std::to_string(kMkDepth);
    return VG_E_ARG;
  }
  int n = 0;
  VG_TRY(used_nodes(ctx, &n));
  // straight after a checkpoint load the flags are the saver's: enabling continues its event stream
  const bool keep = on && ctx->mk_keep;
  ctx->mk_keep = false;
  if (n > 0 && !keep) k_mk_clear<<<grid_for(n), kBlock, 0, ctx->stream>>>(ctx->map, n);
  VG_HIP(hipGetLastError());
  VG_HIP(hipStreamSynchronize(ctx->stream));
  ctx->d_mk.release();
  ctx->d_mk_cnt.release();
  ctx->mk_fresh = false;
  if (!on) return VG_OK;
  VG_HIP(ctx->d_mk.reserve((size_t)ctx->mk_cap));
  VG_HIP(ctx->d_mk_cnt.reserve(4));
  VG_HIP(hipMemset(ctx->d_mk_cnt, 0, 4 * sizeof(int)));
  return VG_OK;
}

int markers_collect(vg_ctx* ctx) {
  hipStream_t s = ctx->stream;
  VG_HIP(hipMemsetAsync(ctx->d_mk_cnt, 0, sizeof(int), s));
  k_mk_collect<<<kMkGrid, kBlock, 0, s>>>(ctx->map, ctx->cfg.max_layer, ctx->d_mk, ctx->mk_cap, ctx->d_mk_cnt);
  VG_HIP(hipGetLastError());
  ctx->mk_fresh = true;
  return VG_OK;
}

// the caller has completed the outstanding work (vg_markers)
int markers_read(vg_ctx* ctx, vg_plane_marker* out, int cap, int* n, int* deferred) {
  int total = 0;
  if (ctx->d_mk_cnt && ctx->mk_fresh) VG_HIP(hipMemcpy(&total, ctx->d_mk_cnt, sizeof(int), hipMemcpyDeviceToHost));
  const int emitted = total < ctx->mk_cap ? total : ctx->mk_cap;
  *n = emitted;
  if (deferred) *deferred = total - emitted;
  const int k = emitted < cap ? emitted : cap;
  if (k > 0) VG_HIP(hipMemcpy(out, ctx->d_mk, (size_t)k * sizeof(vg_plane_marker), hipMemcpyDeviceToHost));
  return VG_OK;
}

// the caller has completed the outstanding work (vg_map_planes)
int map_planes(vg_ctx* ctx, int flags, vg_plane_marker* out, int cap, int* n) {
  if (ctx->cfg.max_layer >= kMkDepth) {
    ctx->err = "vg_map_planes needs max_layer < " + std::to_string(kMkDepth);
    return VG_E_ARG;
  }
  hipStream_t s = ctx->stream;
  int nn = 0;
  VG_TRY(used_nodes(ctx, &nn));
  const int k = out ? cap : 0;
  DevBuf<char> buf;  // the count, then the records
  const size_t off = 256;
  hipError_t e = buf.reserve(off + (size_t)(k > 0 ? k : 1) * sizeof(vg_plane_marker));
  if (e == hipSuccess) e = hipMemsetAsync(buf, 0, off, s);
  int total = 0;
  if (e == hipSuccess) {
    k_mk_snapshot<<<grid_for((long)ctx->map.hash_mask + 1, kBlock, 2048), kBlock, 0, s>>>(
        ctx->map, nn, ctx->cfg.max_layer, flags, k > 0 ? (vg_plane_marker*)(buf + off) : nullptr, k, (int*)buf.p);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&total, buf, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  const int c = total < k ? total : k;
  if (e == hipSuccess && c > 0) e = hipMemcpy(out, buf + off, (size_t)c * sizeof(vg_plane_marker), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    ctx->err = std::string("vg_map_planes: ") + hipGetErrorString(e);
    return VG_E_HIP;
  }
  *n = total;
  return VG_OK;
}

}  // namespace vg

// Test-only: marker_eval as compiled for the device on n caller-supplied
// inputs (15 doubles each: voxel_center 3, layer, quater_length, center 3,
// normal 3, trace, eig 3) -> n records (action 0, flags 0)
extern "C" int vgx_marker_eval(vg_ctx* ctx, const double* in, int n, vg_plane_marker* out) {
  using namespace vg;
  if (!ctx || !in || !out || n <= 0 || n > (1 << 20)) return VG_E_ARG;
  VG_TRY(host_sync(ctx));
  const size_t nin = (size_t)n * kMkEvalIn * sizeof(double), nout = (size_t)n * sizeof(vg_plane_marker);
  DevBuf<double> d_in;
  DevBuf<vg_plane_marker> d_out;
  hipError_t e = d_in.reserve((size_t)n * kMkEvalIn);
  if (e == hipSuccess) e = d_out.reserve((size_t)n);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, nin, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // (the context's stream does not wait for the null stream)
  if (e == hipSuccess) {
    k_mk_eval<<<(n + kBlock - 1) / kBlock, kBlock, 0, ctx->stream>>>(d_in, n, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    ctx->err = std::string("vgx_marker_eval: ") + hipGetErrorString(e);
    return VG_E_HIP;
  }
  return VG_OK;
}
// Test-only: sizeof(vg_plane_marker) as the library was compiled
extern "C" int vgx_marker_sizeof(void) { return (int)sizeof(vg_plane_marker); }
