// occupancy.hip — the 2-D occupancy grid ray-cast from the voxel map
// (vg_occupancy; vina_gpu.h "Occupancy grid"): M origins x D shared directions
// traced through vg_ray.h and rasterised on the device (vg_occ.h), so that only
// the grid, the optional count planes and a 128-byte summary leave it.
//
// k_occ_cast: one lane per (place, direction), lane i = place D + direction,
// 256-thread workgroups, no LDS. ray_trace is the latency-bound gather it is in
// k_raycast; the walk behind it is arithmetic in registers and one int32
// atomicAdd per marked cell. The lanes of a wave share an origin (D >= 64), so
// their first cells coincide and the cell under the sensor takes D atomics per
// place; they are not merged within the wave (DESIGN.md §6 has the measurement).
// The summary's ray counts: one 64-bit atomic per wave and count that occurs.
//
// k_occ_classify: one lane per cell; writes the grid and adds the wave's class
// counts and the two planes' sums to the summary, one atomic per wave each.
//
// Every sum is an integer atomic: the planes, the grid and the summary do not
// depend on the order of the rays or on how M is cut into launches.
#include "vg_occ.h"
#include "vg_query.h"
#include "vg_reduce.h"

namespace vg {

// the summary's int64 slots as the kernels index them (vg_occ_summary's order)
enum { kOccRays = 0, kOccHits, kOccInBand, kOccTrunc, kOccOccupied, kOccInvalid, kOccFreeMarks, kOccOccMarks,
       kOccCellsFree, kOccCellsOccupied, kOccCellsUnknown };

__global__ void __launch_bounds__(kOccBlock) k_occ_cast(double vs, DevMap m, const double* __restrict__ pos,
                                                        const double* __restrict__ dirs, int D, int n, OccPrm prm,
                                                        int* __restrict__ n_free, int* __restrict__ n_occ,
                                                        unsigned long long* __restrict__ sum) {
  const int i = blockIdx.x * kOccBlock + threadIdx.x;
  const bool valid = i < n;
  int flags = 0;
  bool in_band = false;
  if (valid) {
    const int place = i / D, k = i - place * D;
    const V3 o = ld_v3(pos + 3 * (size_t)place), dir = ld_v3(dirs + 3 * (size_t)k);
    vg_ray_hit h;
    ray_trace(m, vs, o, dir, prm.ray, h);
    flags = h.flags;
    occ_ray(prm, o, dir, h, n_free, n_occ, in_band);
  }
  wave_count_add(sum, kOccHits, valid && (flags & kRayHit));
  wave_count_add(sum, kOccInBand, in_band);
  wave_count_add(sum, kOccTrunc, valid && (flags & kRayTruncated));
  wave_count_add(sum, kOccOccupied, valid && (flags & kRayOccupied));
  wave_count_add(sum, kOccInvalid, valid && (flags & kRayInvalid));
}

__global__ void __launch_bounds__(kOccBlock) k_occ_classify(const int* __restrict__ n_free,
                                                            const int* __restrict__ n_occ, int cells, int min_occ,
                                                            int min_free, double occ_ratio,
                                                            int8_t* __restrict__ grid,
                                                            unsigned long long* __restrict__ sum) {
  const int i = blockIdx.x * kOccBlock + threadIdx.x;
  int f = 0, o = 0, cls = 1;  // cls: the lanes past the last cell count nowhere
  if (i < cells) {
    f = n_free[i];
    o = n_occ[i];
    if (o >= min_occ && (double)o >= occ_ratio * ((double)o + (double)f)) cls = VG_OCC_OCCUPIED;
    else cls = f >= min_free ? VG_OCC_FREE : VG_OCC_UNKNOWN;
    grid[i] = (int8_t)cls;
  }
  wave_count_add(sum, kOccCellsFree, cls == VG_OCC_FREE);
  wave_count_add(sum, kOccCellsOccupied, cls == VG_OCC_OCCUPIED);
  wave_count_add(sum, kOccCellsUnknown, cls == VG_OCC_UNKNOWN);
  // the planes' sums, in 64 bits: 64 counts of up to M D each
  const unsigned long long sf = wave_sum((unsigned long long)f), so = wave_sum((unsigned long long)o);
  if ((threadIdx.x & 63) == 0) {
    if (sf) atomicAdd(&sum[kOccFreeMarks], sf);
    if (so) atomicAdd(&sum[kOccOccMarks], so);
  }
}

// ---- host side

static int occ_bufs(vg_ctx* ctx, size_t cells) {
  OccBufs& b = ctx->occ;
  static_assert(sizeof(vg_occ_params) == 176 && sizeof(vg_occ_summary) == 128, "the records' documented sizes");
  b.nx = b.ny = 0;  // (no grid to hand to vg_clearance until this call has finished)
  VG_HIP(b.pos.reserve((size_t)kInfoSlab * 3));
  VG_HIP(b.dirs.reserve((size_t)kInfoMaxDirs * 3));
  VG_HIP(b.sum.reserve(1));
  VG_HIP(b.planes.reserve(2 * cells));
  VG_HIP(b.grid.reserve(cells));
  return VG_OK;
}

int occupancy_dev(vg_ctx* ctx, const MP& mp, const double* positions, int M, const double* dirs, int D,
                  const vg_occ_params* prm, int8_t* grid, int32_t* counts, vg_occ_summary* out) {
  const size_t cells = (size_t)prm->nx * (size_t)prm->ny;
  VG_TRY(occ_bufs(ctx, cells));
  OccBufs& b = ctx->occ;
  hipStream_t s = ctx->stream;
  const OccPrm q = occ_prm(prm);
  unsigned long long* d_sum = reinterpret_cast<unsigned long long*>(b.sum.p);
  int* d_free = b.planes;
  int* d_occ = b.planes + cells;
  b.t.clear();
  VG_HIP(hipMemsetAsync(b.planes, 0, 2 * cells * sizeof(int), s));
  VG_HIP(hipMemsetAsync(d_sum, 0, sizeof(vg_occ_summary), s));
  if (M > 0) VG_HIP(hipMemcpyAsync(b.dirs, dirs, (size_t)D * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  VG_TRY(ray_slabs(ctx, positions, M, D, b.t, [&](int m, int n) {
    k_occ_cast<<<(n + kOccBlock - 1) / kOccBlock, kOccBlock, 0, s>>>(mp.vs, ctx->map, b.pos, b.dirs, D, n, q, d_free,
                                                                     d_occ, d_sum);
  }));
  VG_HIP(b.t.begin(s));
  k_occ_classify<<<(int)((cells + kOccBlock - 1) / kOccBlock), kOccBlock, 0, s>>>(d_free, d_occ, (int)cells, q.min_occ,
                                                                                  q.min_free, q.occ_ratio, b.grid, d_sum);
  VG_HIP(b.t.end(s));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(grid, b.grid, cells, hipMemcpyDeviceToHost, s));
  if (counts) VG_HIP(hipMemcpyAsync(counts, b.planes, 2 * cells * sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(out, d_sum, sizeof(vg_occ_summary), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  VG_HIP(b.t.collect());
  out->n_rays = (int64_t)M * (int64_t)D;
  b.nx = prm->nx, b.ny = prm->ny;
  return VG_OK;
}

}  // namespace vg

// Measurement hook: the device time of the last vg_occupancy call's kernels, summed over its slabs and the
// classification (HIP events on the context stream around them)
extern "C" int vgx_occ_ms(vg_ctx* ctx, double* ms) {
  if (!ctx || !ms || !ctx->occ.t.armed()) return VG_E_ARG;
  *ms = ctx->occ.t.ms;
  return VG_OK;
}
