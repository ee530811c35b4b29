// terrain.hip — the terrain layer ray-cast from the voxel map (vg_terrain;
// vina_gpu.h "Terrain layer"): M origins x D shared directions traced twice
// through vg_ray.h, the per-ray bodies in vg_terrain.h. Only the grid, the
// planes asked for and a 128-byte summary leave the device.
//
// k_ter_ground: one lane per (place, direction) as k_occ_cast, 256-thread
// workgroups, no LDS: the trace, then at most four atomics on the hit's cell
// (int32 add, native 64-bit add, int32 min and max). The summary's ray counts are
// taken here, one 64-bit atomic per wave and count that occurs.
//
// k_ter_cells: one workgroup per tile of 32 x 8 cells. A cell's elevation is one
// 64-bit division; its step needs the eight neighbours', which are recomputed
// from g_n and g_sum in L2 (a cell without ground costs its g_n alone). A variant
// that staged the tile and a one-cell halo in LDS was measured and was not
// faster, so it is not here. cells_ground, max_step and
// max_spread: a wave reduction, LDS atomics across the four waves, one global
// atomic per workgroup and value.
//
// k_ter_marks: the trace again, then the walk with the ground reference: one
// elev load and one quantisation per piece, one int32 atomicAdd per free piece.
//
// k_ter_classify: vg_occupancy's rule per cell, then the step rule. At most 2,048
// workgroups stride over the cells and add their six sums once each: with one
// lane per cell and one atomic per wave, a 4096 x 4096 grid put 262,144 adds on
// the one word that counts the unknown cells (k_occ_classify's shape; DESIGN.md §6
// has what that costs).
//
// Every sum is an integer atomic, min and max commute: no output depends on the
// order of the rays or on how M is cut into launches.
#include "vg_query.h"
#include "vg_reduce.h"
#include "vg_terrain.h"

namespace vg {

// the summary's slots as the kernels index them
enum { kTerRays = 0, kTerHits, kTerInBand, kTerTrunc, kTerOccupied, kTerInvalid, kTerGround, kTerOutOfRange,
       kTerCellsGround, kTerMaxStep, kTerMaxSpread, kTerStepLethal, kTerFreeMarks, kTerOccMarks, kTerCellsFree,
       kTerCellsOccupied, kTerCellsUnknown, kTerSlots };
constexpr int kTerTileX = 32, kTerTileY = 8;  // kTerTileX kTerTileY = kOccBlock
static_assert(kTerTileX * kTerTileY == kOccBlock, "one lane per cell of the tile");
constexpr int kTerClassifyBlocks = 2048;  // k_ter_classify's launch at most: 8 workgroups per CU, each striding over the cells

__global__ void __launch_bounds__(kOccBlock) k_ter_ground(double vs, DevMap m, const double* __restrict__ pos,
                                                          const double* __restrict__ dirs, int D, int n, TerPrm prm,
                                                          int* __restrict__ g_n, unsigned long long* __restrict__ g_sum,
                                                          int* __restrict__ g_min, int* __restrict__ g_max,
                                                          unsigned long long* __restrict__ sum) {
  const int i = blockIdx.x * kOccBlock + threadIdx.x;
  const bool valid = i < n;
  int flags = 0;
  bool ground = false, oor = false;
  if (valid) {
    const int place = i / D, k = i - place * D;
    const V3 o = ld_v3(pos + 3 * (size_t)place), dir = ld_v3(dirs + 3 * (size_t)k);
    vg_ray_hit h;
    ray_trace(m, vs, o, dir, prm.ray, h);
    flags = h.flags;
    ter_ground(prm, o, dir, h, g_n, g_sum, g_min, g_max, ground, oor);
  }
  wave_count_add(sum, kTerHits, valid && (flags & kRayHit));
  wave_count_add(sum, kTerTrunc, valid && (flags & kRayTruncated));
  wave_count_add(sum, kTerOccupied, valid && (flags & kRayOccupied));
  wave_count_add(sum, kTerInvalid, valid && (flags & kRayInvalid));
  wave_count_add(sum, kTerGround, ground);
  wave_count_add(sum, kTerOutOfRange, oor);
}

// floor(s / n) where n >= min_ground (>= 1), else none
__device__ __forceinline__ int ter_elev(int n, long long s, int min_ground) {
  if (n < min_ground) return kTerNone;
  long long e = s / n;
  if (s < 0 && e * n != s) e--;
  return (int)e;
}

__global__ void __launch_bounds__(kOccBlock) k_ter_cells(const int* __restrict__ g_n,
                                                         const unsigned long long* __restrict__ g_sum,
                                                         const int* __restrict__ g_min, const int* __restrict__ g_max,
                                                         int nx, int ny, int tiles_x, int min_ground,
                                                         int* __restrict__ elev, int* __restrict__ step,
                                                         unsigned long long* __restrict__ sum) {
  __shared__ int red[3];  // cells with an elevation, the largest step, the largest spread
  const int ty0 = (blockIdx.x / tiles_x) * kTerTileY, tx0 = (blockIdx.x - (blockIdx.x / tiles_x) * tiles_x) * kTerTileX;
  if (threadIdx.x < 3) red[threadIdx.x] = 0;
  __syncthreads();
  const int x = tx0 + threadIdx.x % kTerTileX, y = ty0 + threadIdx.x / kTerTileX;
  int has = 0, st = 0, spread = 0;
  if (x < nx && y < ny) {
    const size_t c = (size_t)y * nx + x;
    const int n = g_n[c];
    const int e = ter_elev(n, (long long)g_sum[c], min_ground);
    if (n > 0) spread = g_max[c] - g_min[c];
    if (e != kTerNone) {
      has = 1;
#pragma unroll
      for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
          const int xx = x + dx, yy = y + dy;
          if ((dx == 0 && dy == 0) || xx < 0 || xx >= nx || yy < 0 || yy >= ny) continue;
          const size_t cc = (size_t)yy * nx + xx;
          const int f = ter_elev(g_n[cc], (long long)g_sum[cc], min_ground);
          if (f == kTerNone) continue;
          const int d = e > f ? e - f : f - e;  // (both inside +-2^30)
          st = d > st ? d : st;
        }
    }
    elev[c] = e;
    step[c] = st;
  }
  // the three reductions: wave, LDS across the waves, one global atomic each
  const int cnt = wave_sum(has);
  st = wave_max(st);
  spread = wave_max(spread);
  if ((threadIdx.x & 63) == 0) {
    if (cnt) atomicAdd(&red[0], cnt);
    if (st) atomicMax(&red[1], st);
    if (spread) atomicMax(&red[2], spread);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (red[0]) atomicAdd(&sum[kTerCellsGround], (unsigned long long)red[0]);
    if (red[1]) atomicMax(&sum[kTerMaxStep], (unsigned long long)red[1]);
    if (red[2]) atomicMax(&sum[kTerMaxSpread], (unsigned long long)red[2]);
  }
}

__global__ void __launch_bounds__(kOccBlock) k_ter_marks(double vs, DevMap m, const double* __restrict__ pos,
                                                         const double* __restrict__ dirs, int D, int n, TerPrm prm,
                                                         const int* __restrict__ elev, int* __restrict__ n_free,
                                                         int* __restrict__ n_occ,
                                                         unsigned long long* __restrict__ sum) {
  const int i = blockIdx.x * kOccBlock + threadIdx.x;
  bool in_band = false;
  if (i < n) {
    const int place = i / D, k = i - place * D;
    const V3 o = ld_v3(pos + 3 * (size_t)place), dir = ld_v3(dirs + 3 * (size_t)k);
    vg_ray_hit h;
    ray_trace(m, vs, o, dir, prm.ray, h);
    ter_marks(prm, o, dir, h, elev, n_free, n_occ, in_band);
  }
  wave_count_add(sum, kTerInBand, in_band);
}

__global__ void __launch_bounds__(kOccBlock) k_ter_classify(const int* __restrict__ n_free,
                                                            const int* __restrict__ n_occ,
                                                            const int* __restrict__ elev,
                                                            const int* __restrict__ step, int cells, int min_occ,
                                                            int min_free, double occ_ratio, int step_rule, int smax,
                                                            int8_t* __restrict__ grid,
                                                            unsigned long long* __restrict__ sum) {
  // a lane's six sums over its cells (64 bits: a plane's sum reaches 2^24 counts of up to M D each)
  enum { kLethal = 0, kFree, kOccupied, kUnknown, kFreeMarks, kOccMarks, kSums };
  __shared__ unsigned long long red[kSums];
  if (threadIdx.x < kSums) red[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long a[kSums] = {0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x * kOccBlock + threadIdx.x; i < cells; i += gridDim.x * kOccBlock) {
    const int f = n_free[i], o = n_occ[i];
    int cls;
    if (o >= min_occ && (double)o >= occ_ratio * ((double)o + (double)f)) cls = VG_OCC_OCCUPIED;
    else cls = f >= min_free ? VG_OCC_FREE : VG_OCC_UNKNOWN;
    const bool lethal = step_rule && elev[i] != kTerNone && step[i] > smax;
    if (lethal) cls = VG_OCC_OCCUPIED;
    grid[i] = (int8_t)cls;
    a[kLethal] += lethal;
    a[kFree] += cls == VG_OCC_FREE;
    a[kOccupied] += cls == VG_OCC_OCCUPIED;
    a[kUnknown] += cls == VG_OCC_UNKNOWN;
    a[kFreeMarks] += (unsigned long long)f;
    a[kOccMarks] += (unsigned long long)o;
  }
  // wave, LDS across the four waves, one global atomic per workgroup and sum: a single word takes every
  // workgroup's add, so the launch is held to kTerClassifyBlocks workgroups that stride over the cells
#pragma unroll
  for (int k = 0; k < kSums; k++) {
    a[k] = wave_sum(a[k]);
    if ((threadIdx.x & 63) == 0 && a[k]) atomicAdd(&red[k], a[k]);
  }
  __syncthreads();
  if (threadIdx.x < kSums && red[threadIdx.x]) {
    const int slot[kSums] = {kTerStepLethal, kTerCellsFree, kTerCellsOccupied, kTerCellsUnknown, kTerFreeMarks, kTerOccMarks};
    atomicAdd(&sum[slot[threadIdx.x]], red[threadIdx.x]);
  }
}

// ---- host side

static int ter_bufs(vg_ctx* ctx, size_t cells, bool rays) {
  OccBufs& b = ctx->occ;
  TerBufs& t = ctx->ter;
  static_assert(sizeof(vg_terrain_params) == 224 && sizeof(vg_terrain_summary) == 128, "the records' documented sizes");
  t.nx = t.ny = 0;
  VG_HIP(t.gn.reserve(cells));
  VG_HIP(t.gsum.reserve(cells));
  VG_HIP(t.gmin.reserve(cells));
  VG_HIP(t.gmax.reserve(cells));
  VG_HIP(t.elev.reserve(cells));
  VG_HIP(t.step.reserve(cells));
  VG_HIP(t.sum.reserve(kTerSlots));
  if (!rays) return VG_OK;
  b.nx = b.ny = 0;  // (no grid to hand to vg_clearance until this call has finished)
  VG_HIP(b.pos.reserve((size_t)kInfoSlab * 3));
  VG_HIP(b.dirs.reserve((size_t)kInfoMaxDirs * 3));
  VG_HIP(b.planes.reserve(2 * cells));
  VG_HIP(b.grid.reserve(cells));
  return VG_OK;
}

// k_ter_cells over the ground planes in TerBufs, timed by t[1]
static int ter_cells_launch(vg_ctx* ctx, int nx, int ny, int min_ground) {
  TerBufs& t = ctx->ter;
  hipStream_t s = ctx->stream;
  const int tiles_x = (nx + kTerTileX - 1) / kTerTileX, tiles_y = (ny + kTerTileY - 1) / kTerTileY;
  VG_HIP(t.t[1].begin(s));
  k_ter_cells<<<tiles_x * tiles_y, kOccBlock, 0, s>>>(t.gn, t.gsum, t.gmin, t.gmax, nx, ny, tiles_x, min_ground, t.elev,
                                                      t.step, t.sum);
  VG_HIP(t.t[1].end(s));
  VG_HIP(hipGetLastError());
  return VG_OK;
}

int terrain_dev(vg_ctx* ctx, const MP& mp, const double* positions, int M, const double* dirs, int D,
                const vg_terrain_params* prm, int8_t* grid, int32_t* elev, int32_t* step, int32_t* counts,
                vg_terrain_summary* out) {
  const size_t cells = (size_t)prm->nx * (size_t)prm->ny;
  VG_TRY(ter_bufs(ctx, cells, true));
  OccBufs& b = ctx->occ;
  TerBufs& t = ctx->ter;
  hipStream_t s = ctx->stream;
  const TerPrm q = ter_prm(prm);
  int* d_free = b.planes;
  int* d_occ = b.planes + cells;
  for (KernelTimer& k : t.t) k.clear();
  VG_HIP(hipMemsetAsync(b.planes, 0, 2 * cells * sizeof(int), s));
  VG_HIP(hipMemsetAsync(t.gn, 0, cells * sizeof(int), s));
  VG_HIP(hipMemsetAsync(t.gsum, 0, cells * sizeof(unsigned long long), s));
  VG_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(t.gmin.p), INT32_MAX, cells, s));
  VG_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(t.gmax.p), INT32_MIN, cells, s));
  VG_HIP(hipMemsetAsync(t.sum, 0, kTerSlots * sizeof(unsigned long long), s));
  if (M > 0) VG_HIP(hipMemcpyAsync(b.dirs, dirs, (size_t)D * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  for (int pass = 0; pass < 2; pass++) {
    VG_TRY(ray_slabs(ctx, positions, M, D, t.t[pass ? 2 : 0], [&](int m, int n) {
      if (pass == 0)
        k_ter_ground<<<(n + kOccBlock - 1) / kOccBlock, kOccBlock, 0, s>>>(mp.vs, ctx->map, b.pos, b.dirs, D, n, q, t.gn,
                                                                           t.gsum, t.gmin, t.gmax, t.sum);
      else
        k_ter_marks<<<(n + kOccBlock - 1) / kOccBlock, kOccBlock, 0, s>>>(mp.vs, ctx->map, b.pos, b.dirs, D, n, q, t.elev,
                                                                          d_free, d_occ, t.sum);
    }));
    if (pass == 0) VG_TRY(ter_cells_launch(ctx, q.nx, q.ny, q.min_ground));
  }
  VG_HIP(t.t[3].begin(s));
  const size_t cblocks = (cells + kOccBlock - 1) / kOccBlock;
  k_ter_classify<<<(int)(cblocks < (size_t)kTerClassifyBlocks ? cblocks : (size_t)kTerClassifyBlocks), kOccBlock, 0, s>>>(
      d_free, d_occ, t.elev, t.step, (int)cells, q.min_occ, q.min_free, q.occ_ratio, (q.flags & 2) != 0, q.smax, b.grid,
      t.sum);
  VG_HIP(t.t[3].end(s));
  VG_HIP(hipGetLastError());
  unsigned long long h[kTerSlots];
  VG_HIP(hipMemcpyAsync(grid, b.grid, cells, hipMemcpyDeviceToHost, s));
  if (elev) VG_HIP(hipMemcpyAsync(elev, t.elev, cells * sizeof(int), hipMemcpyDeviceToHost, s));
  if (step) VG_HIP(hipMemcpyAsync(step, t.step, cells * sizeof(int), hipMemcpyDeviceToHost, s));
  if (counts) VG_HIP(hipMemcpyAsync(counts, b.planes, 2 * cells * sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(h, t.sum, sizeof(h), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  VG_HIP(t.t[1].collect());
  VG_HIP(t.t[3].collect());
  out->n_rays = (int64_t)M * (int64_t)D;
  out->n_hits = (int64_t)h[kTerHits], out->n_hits_in_band = (int64_t)h[kTerInBand];
  out->n_truncated = (int64_t)h[kTerTrunc], out->n_occupied_unknown = (int64_t)h[kTerOccupied];
  out->n_invalid = (int64_t)h[kTerInvalid];
  out->n_ground_hits = (int64_t)h[kTerGround], out->n_out_of_range = (int64_t)h[kTerOutOfRange];
  out->cells_ground = (int64_t)h[kTerCellsGround];
  out->max_step = (int32_t)h[kTerMaxStep], out->max_spread = (int32_t)h[kTerMaxSpread];
  out->cells_step_lethal = (int64_t)h[kTerStepLethal];
  out->free_marks = (int64_t)h[kTerFreeMarks], out->occ_marks = (int64_t)h[kTerOccMarks];
  out->cells_free = (int64_t)h[kTerCellsFree], out->cells_occupied = (int64_t)h[kTerCellsOccupied];
  out->cells_unknown = (int64_t)h[kTerCellsUnknown];
  b.nx = t.nx = prm->nx, b.ny = t.ny = prm->ny;
  return VG_OK;
}

}  // namespace vg

// Test and measurement hooks (vina_gpu.h "Terrain layer"), for a context with no work outstanding.
// vgx_ter_ground: the four ground planes the last vg_terrain call left on the device (each nx ny, or null); nx, ny
// other than that call's: VG_E_ARG, and nothing is written.
// vgx_ter_cells: the per-cell stage alone on the given ground planes: elev, step (each nx ny, or null) and
// out3 = cells_ground, max_step, max_spread. It leaves no grid and forgets the last call's planes.
// vgx_ter_ms: the device time of the last vg_terrain call's k_ter_ground, k_ter_cells, k_ter_marks and
// k_ter_classify, the ray kernels summed over their slabs.
extern "C" int vgx_ter_ground(vg_ctx* ctx, int nx, int ny, int32_t* g_n, int64_t* g_sum, int32_t* g_min,
                              int32_t* g_max) {
  if (!ctx) return VG_E_ARG;
  vg::TerBufs& t = ctx->ter;
  if (!t.nx) {
    ctx->err = "vgx_ter_ground: no vg_terrain call left its ground planes on this context";
    return VG_E_STATE;
  }
  if (nx != t.nx || ny != t.ny) return VG_E_ARG;  // (the caller's buffers are nx ny cells)
  const size_t cells = (size_t)t.nx * (size_t)t.ny;
  hipStream_t s = ctx->stream;
  if (g_n) VG_HIP(hipMemcpyAsync(g_n, t.gn, cells * sizeof(int), hipMemcpyDeviceToHost, s));
  if (g_sum) VG_HIP(hipMemcpyAsync(g_sum, t.gsum, cells * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  if (g_min) VG_HIP(hipMemcpyAsync(g_min, t.gmin, cells * sizeof(int), hipMemcpyDeviceToHost, s));
  if (g_max) VG_HIP(hipMemcpyAsync(g_max, t.gmax, cells * sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  return VG_OK;
}
extern "C" int vgx_ter_cells(vg_ctx* ctx, int nx, int ny, int min_ground, const int32_t* g_n, const int64_t* g_sum,
                             const int32_t* g_min, const int32_t* g_max, int32_t* elev, int32_t* step, int64_t* out3) {
  if (!ctx || !g_n || !g_sum || !g_min || !g_max || !out3 || !vg::grid_shape_ok(nx, ny, 0)) return VG_E_ARG;
  const size_t cells = (size_t)nx * (size_t)ny;
  VG_TRY(vg::ter_bufs(ctx, cells, false));
  vg::TerBufs& t = ctx->ter;
  hipStream_t s = ctx->stream;
  VG_HIP(hipMemcpyAsync(t.gn, g_n, cells * sizeof(int), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(t.gsum, g_sum, cells * sizeof(int64_t), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(t.gmin, g_min, cells * sizeof(int), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(t.gmax, g_max, cells * sizeof(int), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemsetAsync(t.sum, 0, vg::kTerSlots * sizeof(unsigned long long), s));
  t.t[1].clear();
  VG_TRY(vg::ter_cells_launch(ctx, nx, ny, min_ground > 0 ? min_ground : 1));
  unsigned long long h[vg::kTerSlots];
  if (elev) VG_HIP(hipMemcpyAsync(elev, t.elev, cells * sizeof(int), hipMemcpyDeviceToHost, s));
  if (step) VG_HIP(hipMemcpyAsync(step, t.step, cells * sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(h, t.sum, sizeof(h), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  VG_HIP(t.t[1].collect());
  out3[0] = (int64_t)h[vg::kTerCellsGround], out3[1] = (int64_t)h[vg::kTerMaxStep], out3[2] = (int64_t)h[vg::kTerMaxSpread];
  return VG_OK;
}
extern "C" int vgx_ter_ms(vg_ctx* ctx, double* ms4) {
  if (!ctx || !ms4 || !ctx->ter.t[1].armed()) return VG_E_ARG;
  for (int k = 0; k < 4; k++) ms4[k] = ctx->ter.t[k].ms;
  return VG_OK;
}
