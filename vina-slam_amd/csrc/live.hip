// live.hip — the live obstacle layer's device side (vina_gpu.h "Live obstacle
// layer"): a scan's obstacle points and clearing beams folded into two int32
// stamp planes beside a private base grid, and the planes composed with the base
// into the grid vg_clearance reads. Two kernels per mark, one per compose.
//
// k_live_points: one lane per point, 256-thread workgroups, no LDS. The point is
// classified by vg_diff.h's diff_point (vg_live.h), so its class and the class
// counts have vg_scan_diff's bits; the lane then writes the 32-byte record: flags
// and the cells of o, e and w, in double. Like k_scan_diff it is a latency-bound
// gather dominated by the ray's walk through the map.
//
// k_live_walk: one lane per record, the lanes of a wave on consecutive points:
// neighbouring beams of a scan line cross neighbouring cells. A lane raises its
// obstacle point's hit cell, then walks its beam's cells c_0 .. c_{n-1} and raises
// their clear cells. It keeps the two remainders of the definition's divisions,
// (2 k a + n) mod 2n, and adds 2a a step: a <= n, so a coordinate moves by at most
// one cell a step and no division is left in the loop. Both coordinates are
// monotonic, so a beam that has passed the grid's far side in its direction of
// travel ends there. Every beam of a scan crosses the cells round the origin, and
// an atomic on one address serialises the wave, so a cell is raised with atomicMax
// only where a plain read finds a value below the stamp (view.hip's k_view_rays
// sets its bitmap the same way). The read may be stale; the planes only grow, so
// that costs a redundant atomic and never a wrong value. The atomic's return tells
// the one lane that raised the cell to the stamp, which counts it.
//
// k_live_compose: a grid-stride pass over the cells: the live rule, the composed
// byte, and the summary's counts through vg_reduce.h's block_add. Integer maxima
// and sums only: no plane, grid or count depends on the order of arrival.
#include <cstddef>
#include <cstring>

#include "vg_live.h"
#include "vg_query.h"
#include "vg_reduce.h"

namespace vg {

constexpr int kLiveBlock = kRayBlock;   // 256 threads
constexpr int kLiveMaxN = 4097;         // a beam's n at most: clear_max / res <= 4096, and the floor's one cell
constexpr int kLiveComposeBlocks = 2048;  // k_live_compose's workgroups at most

// the summary's int64 slots as the kernels index them (vg_live_summary's order)
enum { kLvCls = 0, kLvObstacle = 4, kLvDropped, kLvBeams, kLvLive, kLvCleared, kLvFree, kLvOccupied, kLvUnknown,
       kLvRaised, kLvStamp, kLvCalls, kLvSlots = 16 };

typedef unsigned long long u64;

// x, y, z: the cloud, element i at i * stride
__global__ void __launch_bounds__(kLiveBlock) k_live_points(MP mp, DevMap m, const float* __restrict__ x,
                                                            const float* __restrict__ y, const float* __restrict__ z,
                                                            int stride, int n, Pose12 pose, DiffPrm prm, LivePrm q,
                                                            vg_live_point* __restrict__ recs, int* __restrict__ cls6) {
  const int i = blockIdx.x * kLiveBlock + threadIdx.x;
  const bool valid = i < n;
  int cls = -1, rflags = 0;
  if (valid) {
    const size_t at = (size_t)i * (size_t)stride;
    vg_live_point rec;
    live_point(mp, m, v3(x[at], y[at], z[at]), pose, prm, q, rec, rflags);
    cls = rec.cls;
    recs[i] = rec;
  }
  diff_wave_counts(cls, valid, rflags, cls6);
}

// plane[g] = max(plane[g], stamp); true for the one lane that raised it to the stamp
__device__ __forceinline__ bool live_raise(int* __restrict__ plane, size_t g, int stamp) {
  if (plane[g] >= stamp) return false;
  return atomicMax(&plane[g], stamp) < stamp;
}

__global__ void __launch_bounds__(kLiveBlock) k_live_walk(const vg_live_point* __restrict__ recs, int n_recs, int stamp,
                                                          int nx, int ny, int* __restrict__ hit,
                                                          int* __restrict__ clear, u64* __restrict__ sum) {
  const int i = blockIdx.x * kLiveBlock + threadIdx.x;
  bool obstacle = false, dropped = false, beam = false;
  u64 raised_hit = 0, raised_clear = 0;
  if (i < n_recs) {
    const vg_live_point rec = recs[i];
    if (rec.flags & VG_LIVE_MARKS) {
      obstacle = true;
      if (rec.mx >= 0 && rec.mx < nx && rec.my >= 0 && rec.my < ny)
        raised_hit += live_raise(hit, (size_t)rec.my * nx + rec.mx, stamp);
      else
        dropped = true;
    }
    if (rec.flags & VG_LIVE_CLEARS) {
      beam = true;
      const long long ddx = (long long)rec.bx - rec.ax, ddy = (long long)rec.by - rec.ay;
      const long long lax = ddx < 0 ? -ddx : ddx, lay = ddy < 0 ? -ddy : ddy;
      const long long ln = lax > lay ? lax : lay;
      if (ln <= kLiveMaxN) {  // (a record of vg_live_mark always; a longer beam of a given record clears nothing)
        const int n = (int)ln, ax = (int)lax, ay = (int)lay, n2 = 2 * n;
        const int sx = ddx < 0 ? -1 : 1, sy = ddy < 0 ? -1 : 1;
        int rx = n, ry = n;  // (2 k a + n) mod 2n
        int cx = rec.ax, cy = rec.ay;
        for (int k = 0; k < n; k++) {
          if (cx >= 0 && cx < nx && cy >= 0 && cy < ny) {
            raised_clear += live_raise(clear, (size_t)cy * nx + cx, stamp);
          } else if ((ax && (sx > 0 ? cx >= nx : cx < 0)) || (ay && (sy > 0 ? cy >= ny : cy < 0))) {
            break;  // past the grid on an axis that only moves on
          } else if ((!ax && (cx < 0 || cx >= nx)) || (!ay && (cy < 0 || cy >= ny))) {
            break;  // beside the grid on an axis that does not move
          }
          rx += 2 * ax, ry += 2 * ay;
          if (rx >= n2) rx -= n2, cx += sx;
          if (ry >= n2) ry -= n2, cy += sy;
        }
      }
    }
  }
  wave_count_add(sum, kLvObstacle, obstacle);
  wave_count_add(sum, kLvDropped, dropped);
  wave_count_add(sum, kLvBeams, beam);
  block_add<kLiveBlock>(raised_hit, sum, kLvLive);
  block_add<kLiveBlock>(raised_clear, sum, kLvCleared);
}

// grid-stride over the cells. persist == 0: for ever
__global__ void __launch_bounds__(kLiveBlock) k_live_compose(const int8_t* __restrict__ base,
                                                             const int* __restrict__ hit, const int* __restrict__ clear,
                                                             int cells, int now, int persist, int free_unknown,
                                                             int8_t* __restrict__ out, u64* __restrict__ sum) {
  const int stride = gridDim.x * kLiveBlock;
  u64 n_live = 0, n_clr = 0, n_free = 0, n_occ = 0, n_unk = 0, n_raised = 0;
  for (int i = blockIdx.x * kLiveBlock + threadIdx.x; i < cells; i += stride) {
    const int h = hit[i], c = clear[i];
    const int8_t b = base[i];
    const bool live = h > 0 && h >= c && (persist == 0 || (long long)now - h < (long long)persist);
    const bool cleared = !live && c > 0 && c > h && (persist == 0 || (long long)now - c < (long long)persist);
    int8_t v = b;
    if (live) v = VG_OCC_OCCUPIED;
    else if (free_unknown && cleared && b == VG_OCC_UNKNOWN) v = VG_OCC_FREE;
    out[i] = v;
    n_live += live, n_clr += cleared, n_raised += live && b != VG_OCC_OCCUPIED;
    n_occ += v == VG_OCC_OCCUPIED, n_unk += v == VG_OCC_UNKNOWN;
    n_free += v != VG_OCC_OCCUPIED && v != VG_OCC_UNKNOWN;
  }
  block_add<kLiveBlock>(n_live, sum, kLvLive);
  block_add<kLiveBlock>(n_clr, sum, kLvCleared);
  block_add<kLiveBlock>(n_free, sum, kLvFree);
  block_add<kLiveBlock>(n_occ, sum, kLvOccupied);
  block_add<kLiveBlock>(n_unk, sum, kLvUnknown);
  block_add<kLiveBlock>(n_raised, sum, kLvRaised);
}

// ---- host side

static size_t live_cells(const LiveLayer* L) { return (size_t)L->q.nx * (size_t)L->q.ny; }

int live_clear_dev(vg_ctx* ctx, LiveLayer* L) {
  hipStream_t s = ctx->stream;
  const size_t cells = live_cells(L);
  VG_HIP(hipMemsetAsync(L->hit, 0, cells * sizeof(int), s));
  VG_HIP(hipMemsetAsync(L->clear, 0, cells * sizeof(int), s));
  VG_HIP(hipStreamSynchronize(s));
  return VG_OK;
}

int live_alloc(vg_ctx* ctx, LiveLayer* L, const int8_t* base_grid) {
  static_assert(sizeof(vg_live_summary) == kLvSlots * sizeof(u64), "the summary is the kernels' slots");
  static_assert(offsetof(vg_live_summary, n_obstacle) == kLvObstacle * 8 && offsetof(vg_live_summary, calls) == kLvCalls * 8,
                "the summary's fields in the slots' order");
  const size_t cells = live_cells(L);
  VG_HIP(L->base.reserve(cells));
  VG_HIP(L->hit.reserve(cells));
  VG_HIP(L->clear.reserve(cells));
  VG_HIP(L->sum.reserve(kLvSlots));
  VG_HIP(L->cls.reserve(8));
  VG_HIP(hipMemcpyAsync(L->base, base_grid ? base_grid : ctx->occ.grid.p, cells,
                        base_grid ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
  return live_clear_dev(ctx, L);
}

// k_live_walk over L->rec[0 .. n) at `stamp` between t_walk's events; the caller zeroed L->sum
static int live_walk_launch(vg_ctx* ctx, LiveLayer* L, int n, int stamp) {
  hipStream_t s = ctx->stream;
  VG_HIP(L->t_walk.begin(s));
  if (n > 0)
    k_live_walk<<<(n + kLiveBlock - 1) / kLiveBlock, kLiveBlock, 0, s>>>(L->rec, n, stamp, L->q.nx, L->q.ny, L->hit,
                                                                        L->clear, L->sum);
  VG_HIP(L->t_walk.end(s));
  VG_HIP(hipGetLastError());
  return VG_OK;
}

int live_mark_dev(vg_ctx* ctx, LiveLayer* L, const MP& mp, const float* x, const float* y, const float* z, int stride,
                  bool dev, int n, const double* pose12, int stamp, vg_live_point* per_point, vg_live_summary* out) {
  memset(out, 0, sizeof(*out));
  out->stamp = stamp;
  L->t_mark.clear(), L->t_walk.clear();
  if (n <= 0) return VG_OK;
  VG_TRY(ray_bufs(ctx));
  VG_HIP(L->rec.reserve_pow2((size_t)n));
  hipStream_t s = ctx->stream;
  const DiffPrm q = diff_prm(&L->diff);
  Pose12 pose;
  for (int e = 0; e < 12; e++) pose.v[e] = pose12[e];
  if (!dev) {  // the host cloud, n x 3, into the staging vg_scan_diff uses
    float* d_xyz = reinterpret_cast<float*>(ctx->ray.dir.p);
    VG_HIP(hipMemcpyAsync(d_xyz, x, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s));
    x = d_xyz, y = d_xyz + 1, z = d_xyz + 2;
  }
  u64 h_sum[kLvSlots];
  int h_cls[6];
  VG_HIP(L->t_mark.begin(s));
  VG_HIP(hipMemsetAsync(L->sum, 0, kLvSlots * sizeof(u64), s));
  VG_HIP(hipMemsetAsync(L->cls, 0, 8 * sizeof(int), s));
  k_live_points<<<(n + kLiveBlock - 1) / kLiveBlock, kLiveBlock, 0, s>>>(mp, ctx->map, x, y, z, stride, n, pose, q, L->q,
                                                                        L->rec, L->cls);
  VG_HIP(hipGetLastError());
  VG_TRY(live_walk_launch(ctx, L, n, stamp));
  VG_HIP(L->t_mark.end(s));
  VG_HIP(hipMemcpyAsync(h_sum, L->sum, sizeof(h_sum), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(h_cls, L->cls, sizeof(h_cls), hipMemcpyDeviceToHost, s));
  if (per_point) VG_HIP(hipMemcpyAsync(per_point, L->rec, (size_t)n * sizeof(vg_live_point), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  VG_HIP(L->t_mark.collect());
  VG_HIP(L->t_walk.collect());
  for (int c = 0; c < 4; c++) h_sum[kLvCls + c] = (u64)h_cls[c];
  h_sum[kLvStamp] = (u64)stamp;
  memcpy(out, h_sum, sizeof(*out));
  return VG_OK;
}

int live_walk_dev(vg_ctx* ctx, LiveLayer* L, const vg_live_point* recs, int n, int stamp) {
  hipStream_t s = ctx->stream;
  L->t_walk.clear();
  if (n <= 0) return VG_OK;
  VG_HIP(L->rec.reserve_pow2((size_t)n));
  VG_HIP(hipMemcpyAsync(L->rec, recs, (size_t)n * sizeof(vg_live_point), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemsetAsync(L->sum, 0, kLvSlots * sizeof(u64), s));
  VG_TRY(live_walk_launch(ctx, L, n, stamp));
  VG_HIP(hipStreamSynchronize(s));
  VG_HIP(L->t_walk.collect());
  return VG_OK;
}

int live_compose_dev(vg_ctx* ctx, LiveLayer* L, int now, int flags, int8_t* grid, vg_live_summary* out) {
  hipStream_t s = ctx->stream;
  const size_t cells = live_cells(L);
  OccBufs& b = ctx->occ;
  b.nx = b.ny = 0;  // (no grid to hand to vg_clearance until this call has finished)
  VG_HIP(b.grid.reserve(cells));
  u64 h_sum[kLvSlots];
  const size_t want = (cells + kLiveBlock - 1) / kLiveBlock;
  L->t_comp.clear();
  VG_HIP(L->t_comp.begin(s));
  VG_HIP(hipMemsetAsync(L->sum, 0, kLvSlots * sizeof(u64), s));
  k_live_compose<<<(unsigned)(want < (size_t)kLiveComposeBlocks ? want : (size_t)kLiveComposeBlocks), kLiveBlock, 0,
                   s>>>(L->base, L->hit, L->clear, (int)cells, now, L->q.persist, flags & 1, b.grid, L->sum);
  VG_HIP(L->t_comp.end(s));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(h_sum, L->sum, sizeof(h_sum), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  VG_HIP(L->t_comp.collect());
  // (into the caller's arrays only once the kernel ran: a failed launch writes nothing)
  if (grid) {
    VG_HIP(hipMemcpyAsync(grid, b.grid, cells, hipMemcpyDeviceToHost, s));
    VG_HIP(hipStreamSynchronize(s));
  }
  b.nx = L->q.nx, b.ny = L->q.ny;
  if (out) {
    h_sum[kLvStamp] = (u64)now;
    memcpy(out, h_sum, sizeof(*out));
  }
  return VG_OK;
}

}  // namespace vg

// Test / measurement hooks. vgx_live_walk: k_live_walk alone on n given records at `stamp`, into the context's layer
// (a stamp above the layer's largest becomes the largest; the totals are not touched). vgx_live_ms: ms[0] the device
// time of the last vg_live_mark's kernels and the two memsets before them, ms[1] that of its k_live_walk (or of the
// last vgx_live_walk), ms[2] that of the last vg_live_compose (HIP events on the context stream; 0: no such call yet)
extern "C" int vgx_live_walk(vg_ctx* ctx, const vg_live_point* recs, int n, int32_t stamp) {
  if (!ctx || n < 0 || (n > 0 && !recs) || stamp < 1) return VG_E_ARG;
  VG_TRY(vg::query_open(ctx, "vgx_live_walk"));
  vg::LiveLayer* L = ctx->live;
  if (!L) {
    ctx->err = "vgx_live_walk: the context has no live layer (vg_live_begin first)";
    return VG_E_STATE;
  }
  VG_TRY(vg::live_walk_dev(ctx, L, recs, n, stamp));
  if (stamp > L->stamp) L->stamp = stamp;
  return VG_OK;
}
extern "C" int vgx_live_ms(vg_ctx* ctx, double* ms) {
  if (!ctx || !ms) return VG_E_ARG;
  if (!ctx->live) {
    ctx->err = "vgx_live_ms: the context has no live layer (vg_live_begin first)";
    return VG_E_STATE;
  }
  ms[0] = ctx->live->t_mark.ms, ms[1] = ctx->live->t_walk.ms, ms[2] = ctx->live->t_comp.ms;
  return VG_OK;
}
