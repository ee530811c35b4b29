// view.hip — view gain (vg_view_gain; vina_gpu.h "View gain"): the cells a 2-D
// sensor of range R sees from each of n_views cells of the grid, counted by class,
// and what the whole set of viewpoints sees. Two kernels, whatever the input.
//
// k_view_rays: one 256-thread workgroup per viewpoint. A viewpoint outside the
// grid or on an occupied cell writes its record and leaves before any barrier
// (the test is uniform over the workgroup). Otherwise:
//   - the visible set is a bitmap over the viewpoint's window of W x W cells, W =
//     2R + 1, bit wy W + wx, in dynamic LDS: ceil(W^2 / 32) words, 36 bytes at R =
//     1 and 32,644 at R = 255; the launch sizes it by the radius;
//   - with kStage the window's classes (2 bits a cell: free, unknown, occupied;
//     what lies outside the grid is never read) are staged behind the bitmap, a
//     cell a lane, so that a wave reads 64 consecutive cells of a window row.
//     Bitmap and classes take 3 W^2 / 8 bytes, which fits 64 KB up to R = 208; the
//     host launches the variant without staging above that. Which of the two runs
//     below it is ViewBufs::stage (DESIGN.md §5 has the measurement);
//   - the 8R rays go round the window's rim in order, ray t to lane t mod 256, so
//     that the lanes of a wave walk neighbouring rays: they read neighbouring cells
//     and mostly end together. A ray keeps the two remainders of the definition's
//     divisions, (2 k a + n) mod 2n, and adds 2a a step: a <= n, so a coordinate
//     moves by at most one cell a step, and no division is left in the loop;
//   - a visible cell's bit is set with an LDS atomic OR, but only where a plain
//     read finds it clear: all 8R rays cross the cells round the origin, and an
//     atomic on one address serialises the wave. The read may be stale; then the
//     OR sets a bit that is set already;
//   - after a barrier the workgroup walks the bitmap's words, a word a lane:
//     every set bit is one visible cell, classed by the grid (or the staged
//     classes) and added to the device's seen plane with a global integer atomic.
//     The counts are summed per wave by shuffles, per workgroup through LDS, and
//     lane 0 writes the record.
// k_view_sum: a grid-stride pass over the seen plane (cells_seen, unknown_seen)
// and over the records (the status counts, rays, and the best viewpoint as one
// 64-bit atomic max on n_unknown << 32 | ~index: the largest gain, among equals
// the smallest index), one atomic per workgroup and count. Integer sums and
// maxima only: nothing depends on the order in which workgroups arrive.
#include <cstddef>

#include "vg_query.h"
#include "vg_reduce.h"

namespace vg {

constexpr int kViewBlock = 256;
constexpr int kViewWaves = kViewBlock / 64;
constexpr int kViewSumBlocks = 1024;            // k_view_sum's workgroups at most
constexpr size_t kViewLdsMax = 64 * 1024 - 256;  // dynamic LDS of k_view_rays at most (its static part: 64 bytes)
enum { kViewFree = 0, kViewUnknown = 1, kViewOccupied = 2 };

// the summary's int64 slots as the kernels index them (vg_view_summary's order); kViewKey: the best viewpoint's key
enum { kVwViews = 0, kVwOk, kVwOutside, kVwBlocked, kVwRays, kVwMaxUnknown, kVwBest, kVwCells, kVwUnknown,
       kVwKey = 16, kVwSlots = 17 };

typedef unsigned long long u64;

__device__ __forceinline__ int view_class(int8_t v) {
  return v == VG_OCC_OCCUPIED ? kViewOccupied : v == VG_OCC_UNKNOWN ? kViewUnknown : kViewFree;
}
__device__ __forceinline__ int view_staged(const unsigned* s_cls, int idx) {
  return (s_cls[idx >> 4] >> ((idx & 15) * 2)) & 3;
}

// grid: n_views workgroups; dynamic LDS: n_bm words, with kStage another ceil(W^2 / 16)
template <bool kStage>
__global__ void __launch_bounds__(kViewBlock) k_view_rays(const int8_t* __restrict__ grid, int nx, int ny, int R,
                                                          int max_unknown, const int* __restrict__ views, int n_bm,
                                                          vg_view_rec* __restrict__ recs, int* __restrict__ seen) {
  extern __shared__ unsigned s_dyn[];
  __shared__ int s_red[kViewWaves][4];
  unsigned* s_bm = s_dyn;
  unsigned* s_cls = s_dyn + n_bm;
  const int tid = threadIdx.x;
  const int ox = views[2 * blockIdx.x], oy = views[2 * blockIdx.x + 1];
  vg_view_rec rec;
  rec.ix = ox, rec.iy = oy, rec.status = VG_VIEW_OK;
  rec.n_visible = rec.n_unknown = rec.n_free = rec.n_occupied = rec.n_rays_open = 0;
  if (ox < 0 || ox >= nx || oy < 0 || oy >= ny) rec.status = VG_VIEW_OUTSIDE;
  else if (grid[(size_t)oy * nx + ox] == VG_OCC_OCCUPIED) rec.status = VG_VIEW_BLOCKED;
  if (rec.status != VG_VIEW_OK) {  // (uniform over the workgroup: no barrier is skipped by a part of it)
    if (tid == 0) recs[blockIdx.x] = rec;
    return;
  }
  const int W = 2 * R + 1, cells_w = W * W;
  const int x0 = ox - R, y0 = oy - R;  // the window's corner, which may lie outside the grid
  for (int j = tid; j < n_bm; j += kViewBlock) s_bm[j] = 0u;
  if (kStage) {
    // a lane a cell, so that a wave reads 64 consecutive cells of a window row (or the end of one and the start of
    // the next); 16 lanes OR their classes into one word. The trip count is uniform: every lane shuffles
    const int n_cls = (cells_w + 15) >> 4;
    const int dq = kViewBlock / W, dr = kViewBlock - dq * W;  // a step of kViewBlock cells, in rows and cells
    int wy = tid / W, wx = tid - wy * W;
    for (int base = 0; base < n_cls * 16; base += kViewBlock) {
      const int idx = base + tid;
      const int gx = x0 + wx, gy = y0 + wy;
      int c = kViewOccupied;  // (outside the grid or past the window: never read)
      if (idx < cells_w && gx >= 0 && gx < nx && gy >= 0 && gy < ny) c = view_class(grid[(size_t)gy * nx + gx]);
      unsigned word = (unsigned)c << (2 * (tid & 15));
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) word |= __shfl_xor(word, off, 64);
      if ((tid & 15) == 0 && (idx >> 4) < n_cls) s_cls[idx >> 4] = word;
      wx += dr, wy += dq;
      if (wx >= W) wx -= W, wy++;
    }
  }
  __syncthreads();
  if (tid == 0) atomicOr(&s_bm[(R * W + R) >> 5], 1u << ((R * W + R) & 31));  // the origin's own cell
  // the class of the cell at (cx, cy), inside the grid and the window; idx: its bit, wy W + wx
  const auto cls = [&](int cx, int cy, int idx) {
    return kStage ? view_staged(s_cls, idx) : view_class(grid[(size_t)cy * nx + cx]);
  };
  int n_open = 0;
  const int n2 = 2 * R, r2 = R * R;
  for (int t = tid; t < 8 * R; t += kViewBlock) {
    // the rim, clockwise from the corner (-R, -R): four sides of 2R targets, each without its last corner
    const int side = t / n2, j = t - side * n2;
    const int dx = side == 0 ? j - R : side == 1 ? R : side == 2 ? R - j : -R;
    const int dy = side == 0 ? -R : side == 1 ? j - R : side == 2 ? R : R - j;
    const int ax = abs(dx), ay = abs(dy), sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
    int rx = R, ry = R;          // (2 k a + n) mod 2n
    int px = 0, py = 0;          // |c_k - origin| per axis
    int cx = ox, cy = oy, idx = R * W + R;
    int u = 0;
    bool open = true;
    for (int k = 1; k <= R; k++) {
      rx += 2 * ax, ry += 2 * ay;
      const bool mx = rx >= n2, my = ry >= n2;
      const int qx = cx, qy = cy, qidx = idx;  // c_{k-1}
      if (mx) rx -= n2, px++, cx += sx, idx += sx;
      if (my) ry -= n2, py++, cy += sy, idx += sy * W;
      if (cx < 0 || cx >= nx || cy < 0 || cy >= ny) break;
      if (px * px + py * py > r2) break;
      if (mx && my && cls(qx, cy, qidx + sy * W) == kViewOccupied && cls(cx, qy, qidx + sx) == kViewOccupied) {
        open = false;
        break;
      }
      const unsigned bit = 1u << (idx & 31);
      if (!(s_bm[idx >> 5] & bit)) atomicOr(&s_bm[idx >> 5], bit);
      const int c = cls(cx, cy, idx);
      if (c == kViewOccupied) {
        open = false;
        break;
      }
      if (c == kViewUnknown && ++u >= max_unknown && max_unknown > 0) break;
    }
    n_open += open;
  }
  __syncthreads();
  int n_unk = 0, n_free = 0, n_occ = 0;
  for (int j = tid; j < n_bm; j += kViewBlock) {
    unsigned bits = s_bm[j];
    if (!bits) continue;
    const int wy0 = (j * 32) / W, wx0 = j * 32 - wy0 * W;
    while (bits) {
      const int b = __ffs(bits) - 1;
      bits &= bits - 1u;
      int wx = wx0 + b, wy = wy0;
      while (wx >= W) wx -= W, wy++;
      const size_t g = (size_t)(y0 + wy) * nx + (x0 + wx);  // (a visible cell lies inside the grid)
      const int c = kStage ? view_staged(s_cls, j * 32 + b) : view_class(grid[g]);
      n_unk += c == kViewUnknown, n_free += c == kViewFree, n_occ += c == kViewOccupied;
      atomicAdd(&seen[g], 1);
    }
  }
  n_unk = wave_sum(n_unk), n_free = wave_sum(n_free), n_occ = wave_sum(n_occ);
  n_open = wave_sum(n_open);
  if ((tid & 63) == 0) {
    int* r = s_red[tid >> 6];
    r[0] = n_unk, r[1] = n_free, r[2] = n_occ, r[3] = n_open;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 0; w < kViewWaves; w++) {
      rec.n_unknown += s_red[w][0], rec.n_free += s_red[w][1], rec.n_occupied += s_red[w][2];
      rec.n_rays_open += s_red[w][3];
    }
    rec.n_visible = rec.n_unknown + rec.n_free + rec.n_occupied;
    recs[blockIdx.x] = rec;
  }
}

// grid-stride over the cells and over the records
__global__ void __launch_bounds__(kViewBlock) k_view_sum(const int8_t* __restrict__ grid, const int* __restrict__ seen,
                                                         int cells, const vg_view_rec* __restrict__ recs, int n_views,
                                                         int R, u64* __restrict__ sum) {
  const int stride = gridDim.x * kViewBlock, first = blockIdx.x * kViewBlock + threadIdx.x;
  u64 n_seen = 0, n_unk = 0;
  for (int i = first; i < cells; i += stride)
    if (seen[i] > 0) n_seen++, n_unk += grid[i] == VG_OCC_UNKNOWN;
  u64 n_ok = 0, n_out = 0, n_blk = 0, key = 0;
  for (int i = first; i < n_views; i += stride) {
    const int st = recs[i].status;
    n_ok += st == VG_VIEW_OK, n_out += st == VG_VIEW_OUTSIDE, n_blk += st == VG_VIEW_BLOCKED;
    if (st == VG_VIEW_OK) {
      const u64 k = (u64)(unsigned)recs[i].n_unknown << 32 | (u64)(0xFFFFFFFFu - (unsigned)i);  // (never 0)
      key = k > key ? k : key;
    }
  }
  block_add<kViewBlock>(n_seen, sum, kVwCells);
  block_add<kViewBlock>(n_unk, sum, kVwUnknown);
  block_add<kViewBlock>(n_ok, sum, kVwOk);
  block_add<kViewBlock>(n_ok * (u64)(8 * R), sum, kVwRays);
  block_add<kViewBlock>(n_out, sum, kVwOutside);
  block_add<kViewBlock>(n_blk, sum, kVwBlocked);
  key = wave_max(key);
  if ((threadIdx.x & 63) == 0 && key) atomicMax(&sum[kVwKey], key);
}

// ---- host side

int view_gain_dev(vg_ctx* ctx, const int8_t* grid, const vg_view_params* prm, const int32_t* views, int n_views,
                  vg_view_rec* recs, int32_t* seen, vg_view_summary* out) {
  const int nx = prm->nx, ny = prm->ny, R = prm->radius;
  const size_t cells = (size_t)nx * (size_t)ny;
  const int W = 2 * R + 1;
  const int n_bm = (W * W + 31) / 32, n_cls = (W * W + 15) / 16;
  ViewBufs& b = ctx->view;
  VG_HIP(b.sum.reserve(kVwSlots));
  VG_HIP(b.views.reserve(2 * (size_t)VG_NAV_MAX_POINTS));
  VG_HIP(b.rec.reserve_pow2((size_t)n_views));
  VG_HIP(b.seen.reserve(cells));
  if (grid) VG_HIP(b.grid.reserve(cells));
  hipStream_t s = ctx->stream;
  const int8_t* d_grid;
  const bool stage = b.stage && (size_t)(n_bm + n_cls) * sizeof(unsigned) <= kViewLdsMax;
  const size_t lds = (size_t)(n_bm + (stage ? n_cls : 0)) * sizeof(unsigned);
  static_assert((size_t)((2 * VG_VIEW_MAX_RADIUS + 1) * (2 * VG_VIEW_MAX_RADIUS + 1) + 31) / 32 * sizeof(unsigned) <=
                    kViewLdsMax, "the bitmap of the largest radius fits the LDS of a workgroup");
  u64 h_sum[kVwSlots];
  b.t.clear();
  VG_TRY(plane_in(ctx, grid, b.grid, ctx->occ.grid.p, cells, &d_grid));
  VG_HIP(hipMemcpyAsync(b.views, views, 2 * (size_t)n_views * sizeof(int), hipMemcpyHostToDevice, s));
  VG_HIP(b.t.begin(s));
  VG_HIP(hipMemsetAsync(b.sum, 0, kVwSlots * sizeof(u64), s));
  VG_HIP(hipMemsetAsync(b.seen, 0, cells * sizeof(int), s));
  if (stage)
    k_view_rays<true><<<(unsigned)n_views, kViewBlock, lds, s>>>(d_grid, nx, ny, R, prm->max_unknown, b.views, n_bm,
                                                                  b.rec, b.seen);
  else
    k_view_rays<false><<<(unsigned)n_views, kViewBlock, lds, s>>>(d_grid, nx, ny, R, prm->max_unknown, b.views, n_bm,
                                                                   b.rec, b.seen);
  VG_HIP(hipGetLastError());
  const size_t lanes = cells > (size_t)n_views ? cells : (size_t)n_views;
  const size_t want = (lanes + kViewBlock - 1) / kViewBlock;
  k_view_sum<<<(unsigned)(want < (size_t)kViewSumBlocks ? want : (size_t)kViewSumBlocks), kViewBlock, 0, s>>>(
      d_grid, b.seen, (int)cells, b.rec, n_views, R, b.sum);
  VG_HIP(b.t.end(s));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(h_sum, b.sum, sizeof(h_sum), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  VG_HIP(b.t.collect());
  // (into the caller's arrays only once every kernel ran: a failed launch writes nothing)
  VG_HIP(hipMemcpyAsync(recs, b.rec, (size_t)n_views * sizeof(vg_view_rec), hipMemcpyDeviceToHost, s));
  if (seen) VG_HIP(hipMemcpyAsync(seen, b.seen, cells * sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  const u64 key = h_sum[kVwKey];
  h_sum[kVwViews] = (u64)n_views;
  h_sum[kVwMaxUnknown] = key >> 32;
  h_sum[kVwBest] = key ? (u64)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)) : (u64)-1ll;
  memcpy(out, h_sum, sizeof(vg_view_summary));
  return VG_OK;
}

}  // namespace vg

// Measurement hooks. vgx_view_ms: the device time of the last vg_view_gain call's kernels and the two memsets before
// them (HIP events on the context stream). vgx_view_stage: whether k_view_rays stages the window's classes in LDS
// where bitmap and classes fit; the outputs are the same bytes either way
extern "C" int vgx_view_ms(vg_ctx* ctx, double* ms) {
  if (!ctx || !ms || !ctx->view.t.armed()) return VG_E_ARG;
  *ms = ctx->view.t.ms;
  return VG_OK;
}
extern "C" int vgx_view_stage(vg_ctx* ctx, int on) {
  if (!ctx) return VG_E_ARG;
  ctx->view.stage = on != 0;
  return VG_OK;
}
