// clearance.hip — the clearance field and costmap of the 2-D grid (vg_clearance;
// vina_gpu.h "Clearance field and costmap"): the exact squared Euclidean
// distance transform, its feature transform and the inflation cost, separable
// and in integers throughout.
//
// k_clr_cols: one lane per column, so that the lanes of a wave read consecutive
// bytes of a row. A down sweep writes every cell the offset to the last obstacle
// above it in the plane dy (int16: oy - iy <= 0, kClrNone: none yet); an up sweep
// reads that plane back and replaces the offset where the next obstacle below is
// strictly nearer, so equal distances keep the smaller iy. Rows go kClrBatch at a
// time, their loads issued together. The lane counts its obstacles and unknown
// cells; one 64-bit atomic per wave and count.
//
// k_clr_rows: one 256-thread workgroup per row, the row's dy staged in LDS (2 nx
// bytes: the widest legal row, 32768 cells, is 64 KB, so no row is cut into
// tiles). A thread owns the cells ix = t, t + 256, ..; per cell it walks k = 0,
// 1, .. over the columns ix -+ k and keeps the lexicographic minimum of (k^2 +
// dy^2, (iy + dy) nx + x'), until k^2 exceeds the best so far (no farther column
// can beat or tie it, its own k^2 already being larger) or both sides have left
// the row. The cost is one byte looked up by dist2 in the host's table. The
// thread keeps its cells' class counts and largest dist2 in registers; a wave
// adds them up and issues one atomic per count that occurs.
//
// Every loop is bounded by nx or ny; no workgroup waits for another; the only
// atomics are the summary's integer ones.
#include <climits>

#include "vg_query.h"
#include "vg_reduce.h"

namespace vg {

constexpr int kClrBlock = 256;
constexpr int kClrBatch = 8;            // rows per batch of k_clr_cols' loads
constexpr int kClrNone = -32768;        // dy: the column holds no obstacle (|oy - iy| <= 32767 otherwise)

// the summary's int64 slots as the kernels index them (vg_clr_summary's order)
enum { kClrObstacles = 0, kClrUnknown, kClrLethal, kClrInscribed, kClrInflated, kClrFree, kClrNoInfo, kClrMaxDist2 };

__device__ __forceinline__ bool clr_obstacle(int v, int unknown_too) {
  return v == VG_OCC_OCCUPIED || (unknown_too && v == VG_OCC_UNKNOWN);
}

__global__ void __launch_bounds__(kClrBlock) k_clr_cols(const int8_t* __restrict__ grid, int nx, int ny,
                                                        int unknown_too, int16_t* dy,
                                                        unsigned long long* __restrict__ sum) {
  const int ix = blockIdx.x * kClrBlock + threadIdx.x;
  unsigned long long n_obst = 0, n_unk = 0;
  if (ix < nx) {
    int last = -1;  // iy of the last obstacle met going down; -1: none
    for (int y0 = 0; y0 < ny; y0 += kClrBatch) {
      int v[kClrBatch];
#pragma unroll
      for (int j = 0; j < kClrBatch; j++) v[j] = y0 + j < ny ? (int)grid[(size_t)(y0 + j) * nx + ix] : 0;
#pragma unroll
      for (int j = 0; j < kClrBatch; j++) {
        const int iy = y0 + j;
        if (iy < ny) {
          n_unk += v[j] == VG_OCC_UNKNOWN;
          if (clr_obstacle(v[j], unknown_too)) last = iy, n_obst++;
          dy[(size_t)iy * nx + ix] = (int16_t)(last >= 0 ? last - iy : kClrNone);
        }
      }
    }
    int next = -1;  // iy of the last obstacle met going up; -1: none
    for (int y1 = ny - 1; y1 >= 0; y1 -= kClrBatch) {
      int d[kClrBatch];
#pragma unroll
      for (int j = 0; j < kClrBatch; j++) d[j] = y1 - j >= 0 ? (int)dy[(size_t)(y1 - j) * nx + ix] : 0;
#pragma unroll
      for (int j = 0; j < kClrBatch; j++) {
        const int iy = y1 - j;
        if (iy >= 0) {
          if (d[j] == 0) next = iy;
          else if (next >= 0 && (d[j] == kClrNone || next - iy < -d[j])) dy[(size_t)iy * nx + ix] = (int16_t)(next - iy);
        }
      }
    }
  }
  n_obst = wave_sum(n_obst);
  n_unk = wave_sum(n_unk);
  if ((threadIdx.x & 63) == 0) {
    if (n_obst) atomicAdd(&sum[kClrObstacles], n_obst);
    if (n_unk) atomicAdd(&sum[kClrUnknown], n_unk);
  }
}

// dynamic LDS: the row's dy, nx int16
__global__ void __launch_bounds__(kClrBlock) k_clr_rows(const int8_t* __restrict__ grid,
                                                        const int16_t* __restrict__ dy, int nx,
                                                        const uint8_t* __restrict__ table, int table_n,
                                                        int* __restrict__ dist2, int* __restrict__ nearest,
                                                        uint8_t* __restrict__ cost,
                                                        unsigned long long* __restrict__ sum) {
  extern __shared__ __attribute__((aligned(16))) int16_t row[];
  const int iy = blockIdx.x;
  const size_t base = (size_t)iy * nx;
  for (int x = threadIdx.x; x < nx; x += kClrBlock) row[x] = dy[base + x];
  __syncthreads();
  unsigned long long n_cls[5] = {0, 0, 0, 0, 0};  // lethal, inscribed, inflated, free, no_info
  unsigned long long d2_max = 0;
  for (int ix = threadIdx.x; ix < nx; ix += kClrBlock) {
    int best = INT_MAX, at = -1;
    {
      const int s = row[ix];
      if (s != kClrNone) best = s * s, at = (iy + s) * nx + ix;
    }
    const int reach = ix > nx - 1 - ix ? ix : nx - 1 - ix;  // the farther end of the row
    for (int k = 1; k <= reach; k++) {
      const int k2 = k * k;
      if (k2 > best) break;
      if (ix - k >= 0) {
        const int s = row[ix - k];
        if (s != kClrNone) {
          const int d = k2 + s * s, i = (iy + s) * nx + ix - k;
          if (d < best || (d == best && i < at)) best = d, at = i;
        }
      }
      if (ix + k < nx) {
        const int s = row[ix + k];
        if (s != kClrNone) {
          const int d = k2 + s * s, i = (iy + s) * nx + ix + k;
          if (d < best || (d == best && i < at)) best = d, at = i;
        }
      }
    }
    int c = at >= 0 && best < table_n ? (int)table[best] : VG_COST_FREE;
    if (grid[base + ix] == VG_OCC_UNKNOWN && c < VG_COST_INSCRIBED) c = VG_COST_NO_INFO;
    if (dist2) dist2[base + ix] = best;
    if (nearest) nearest[base + ix] = at;
    if (cost) cost[base + ix] = (uint8_t)c;
    n_cls[0] += c == VG_COST_LETHAL;
    n_cls[1] += c == VG_COST_INSCRIBED;
    n_cls[2] += c > VG_COST_FREE && c < VG_COST_INSCRIBED;
    n_cls[3] += c == VG_COST_FREE;
    n_cls[4] += c == VG_COST_NO_INFO;
    if (at >= 0 && (unsigned long long)best > d2_max) d2_max = (unsigned long long)best;
  }
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const unsigned long long n = wave_sum(n_cls[j]);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&sum[kClrLethal + j], n);
  }
  d2_max = wave_max(d2_max);
  if ((threadIdx.x & 63) == 0 && d2_max) atomicMax(&sum[kClrMaxDist2], d2_max);
}

// ---- host side

static int clr_bufs(vg_ctx* ctx, size_t cells, bool want_dist2, bool want_nearest, bool want_cost) {
  ClrBufs& b = ctx->clr;
  static_assert(sizeof(vg_clr_params) == 80 && sizeof(vg_clr_summary) == 128, "the records' documented sizes");
  VG_HIP(b.sum.reserve(1));
  bool regrown = false;
  VG_HIP(b.grid.reserve(cells, &regrown));
  if (regrown) {  // the other planes go with it; an output comes back at the new capacity once a call asks for it
    b.dy.release(), b.dist2.release(), b.nearest.release(), b.cost.release();
    b.nx = b.ny = 0;
  }
  VG_HIP(b.dy.reserve(b.grid.cap));
  if (want_dist2) VG_HIP(b.dist2.reserve(b.grid.cap));
  if (want_nearest) VG_HIP(b.nearest.reserve(b.grid.cap));
  if (want_cost) VG_HIP(b.cost.reserve(b.grid.cap));
  return VG_OK;
}

// the cost table on the device is the one these parameters give: kept while they stay
bool clr_table_current(const vg_ctx* ctx, const vg_clr_params* prm, int table_n) {
  const ClrBufs& b = ctx->clr;
  const double key[4] = {prm->res, prm->inscribed_radius, prm->inflation_radius, prm->cost_scaling};
  return b.table_n == table_n && memcmp(b.table_key, key, sizeof(key)) == 0;
}

int clearance_dev(vg_ctx* ctx, const int8_t* grid, const vg_clr_params* prm, const uint8_t* table, int table_n,
                  int32_t* dist2, int32_t* nearest, uint8_t* cost, vg_clr_summary* out) {
  const int nx = prm->nx, ny = prm->ny;
  const size_t cells = (size_t)nx * (size_t)ny;
  VG_TRY(clr_bufs(ctx, cells, dist2 != nullptr, nearest != nullptr, cost != nullptr));
  ClrBufs& b = ctx->clr;
  hipStream_t s = ctx->stream;
  unsigned long long* d_sum = reinterpret_cast<unsigned long long*>(b.sum.p);
  const int8_t* d_grid;
  b.t.clear();
  if (cost) b.nx = b.ny = 0;  // (no cost plane to hand to vg_navfn until this call has finished)
  if (table) {
    const double key[4] = {prm->res, prm->inscribed_radius, prm->inflation_radius, prm->cost_scaling};
    b.table_n = 0;
    VG_HIP(b.table.reserve((size_t)table_n));
    VG_HIP(hipMemcpyAsync(b.table, table, (size_t)table_n, hipMemcpyHostToDevice, s));
    VG_HIP(hipStreamSynchronize(s));  // (the caller's table goes away with the call)
    memcpy(b.table_key, key, sizeof(key));
    b.table_n = table_n;
  }
  VG_TRY(plane_in(ctx, grid, b.grid, ctx->occ.grid.p, cells, &d_grid));
  VG_HIP(hipMemsetAsync(d_sum, 0, sizeof(vg_clr_summary), s));
  VG_HIP(b.t.begin(s));
  k_clr_cols<<<(nx + kClrBlock - 1) / kClrBlock, kClrBlock, 0, s>>>(d_grid, nx, ny, prm->flags & 1, b.dy, d_sum);
  VG_HIP(hipGetLastError());
  k_clr_rows<<<ny, kClrBlock, (size_t)nx * sizeof(int16_t), s>>>(d_grid, b.dy, nx, b.table, table_n,
                                                                   dist2 ? b.dist2.p : nullptr,
                                                                   nearest ? b.nearest.p : nullptr,
                                                                   cost ? b.cost.p : nullptr, d_sum);
  VG_HIP(b.t.end(s));
  VG_HIP(hipGetLastError());
  if (dist2) VG_HIP(hipMemcpyAsync(dist2, b.dist2, cells * sizeof(int), hipMemcpyDeviceToHost, s));
  if (nearest) VG_HIP(hipMemcpyAsync(nearest, b.nearest, cells * sizeof(int), hipMemcpyDeviceToHost, s));
  if (cost) VG_HIP(hipMemcpyAsync(cost, b.cost, cells, hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(out, d_sum, sizeof(vg_clr_summary), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  VG_HIP(b.t.collect());
  if (cost) b.nx = nx, b.ny = ny;
  return VG_OK;
}

}  // namespace vg

// Measurement hook: the device time of the last vg_clearance call's two kernels (HIP events on the context
// stream around them)
extern "C" int vgx_clr_ms(vg_ctx* ctx, double* ms) {
  if (!ctx || !ms || !ctx->clr.t.armed()) return VG_E_ARG;
  *ms = ctx->clr.t.ms;
  return VG_OK;
}
