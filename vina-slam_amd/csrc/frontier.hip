// frontier.hip — exploration frontiers (vg_frontiers; vina_gpu.h "Exploration
// frontiers"): the free cells beside unknown space, labelled into 8-connected
// components by a union-find and summed into one record per component. Seven
// kernels and a scan that runs twice, nine launches in a fixed sequence: the
// launch count does not depend on the input, and no host loop runs rounds.
//
// k_fr_tile: one 256-thread workgroup per tile of kFrTile x kFrTile cells (the
// geometry of k_nav_relax: a thread owns 16 consecutive cells of a column, the
// lanes of a wave 64 consecutive cells of a row). It stages the grid with a
// one-cell halo in LDS for the 4-neighbour test, reads the cost and the potential
// of its own cells, marks the frontier cells and labels them inside the tile by a
// union-find in LDS: every frontier cell is united with its W, NW, N and NE
// neighbour of the tile, which covers each adjacent pair once. It writes
// parent[i], the global linear index of the tile-local minimum (-1 off the
// frontier), and adds the summary's cell counts, one atomic per wave and count.
//
// k_fr_merge: one lane per cell on a tile's low rim (ix % 64 == 0: the three
// neighbours at ix - 1; iy % 64 == 0: the three at iy - 1; between them every
// adjacent pair of cells in different tiles, the diagonals through a corner where
// four tiles meet included). It unites the cell with those that are frontier
// cells, in the global forest.
//
// The union, in LDS and in global memory alike: find both roots; if they differ,
// atomicMin the larger root's parent to the smaller; if the value read back shows
// that another lane moved that root meanwhile, go on with the pair (value read
// back, smaller root). Why this is exact and ends:
//   - a parent is only ever written by atomicMin with a smaller index, and starts
//     as the cell itself or a smaller one: parent[i] <= i at all times, so every
//     find walk strictly descends and ends at a cell with parent[r] == r;
//   - every link joins two cells of one true component, so no tree ever holds
//     cells of two;
//   - take the graph of the forest's links plus, per lane, the pair it still has
//     to unite. An atomicMin that finds the root untouched adds the wanted link.
//     One that finds parent[a] == c != a leaves min(c, b) there and takes on the
//     pair (c, b): a stays joined to b and c through a link and the pending pair.
//     The connectivity of that graph never shrinks. When every lane has returned
//     no pair is pending, so the forest alone connects every pair handed to a
//     union, i.e. every pair of adjacent frontier cells: one tree per component;
//   - a tree's root is no larger than any of its cells, so it is the component's
//     smallest linear index, which is label's definition;
//   - a retry continues with two roots both smaller than the root it lost, so a
//     lane retries fewer times than there are cells. No lane waits for another; a
//     retry happens only because the forest made progress.
// A find may read a link that another lane has since replaced: it then walks a
// path that existed, inside the same component, and the atomicMin (performed at
// the memory, device scope) decides on the current value. In k_fr_merge the walks
// load with agent scope so that they see other workgroups' links soon; in the
// kernels after it the forest is read-only. Every such loop still carries an
// explicit bound (the tile's cells in LDS, nx ny globally); overrunning it raises
// a device flag that turns the call into VG_E_CAPACITY with nothing written.
//
// k_fr_flatten: label[i] = find(i), and per workgroup the number of roots.
// k_fr_scan (one workgroup) turns the at most kFrMaxCounts counts into offsets;
// k_fr_number gives each root its dense id in ascending label order (offset + rank
// among the workgroup's lanes, by ballot), starts its record and leaves the id in
// parent[root]. Nothing depends on the order in which atomics arrive.
// k_fr_stats: one lane per frontier cell into its component's record, integer
// atomics only (add: size, sums; min / max: the box; a 64-bit min on pot << 32 |
// cell: best), so the sums are exact in any order. k_fr_keep, k_fr_scan and
// k_fr_emit filter by min_size with the same ordered compaction and write the
// first max_records records.
#include <climits>
#include <cstddef>

#include "vg_query.h"
#include "vg_reduce.h"

namespace vg {

constexpr int kFrBlock = 256;
constexpr int kFrTile = 64;                        // a tile's side, cells
constexpr int kFrPitch = kFrTile + 2;              // ... with its halo
constexpr int kFrRows = kFrTile * kFrTile / kFrBlock;  // cells of a column that a thread owns
constexpr int kFrMaxCounts = 65536;                // workgroups of one lane per cell at VG_OCC_MAX_CELLS
constexpr unsigned kFrUnreached = VG_NAV_UNREACHED;
static_assert(kFrBlock == 4 * kFrTile && kFrRows == 16, "a thread's run of cells: one column of a quarter tile");
static_assert((size_t)kFrMaxCounts * kFrBlock >= (size_t)VG_OCC_MAX_CELLS, "one count per workgroup of cells");

// the summary's int64 slots as the kernels index them (vg_frontier_summary's order); kFrFlag: a bounded loop ran out
enum { kFrCells = 0, kFrComponents, kFrKept, kFrWritten, kFrMaxSize, kFrFree, kFrUnknown, kFrRejCost, kFrRejUnreached,
       kFrFlag = 16, kFrSlots = 17 };

typedef unsigned long long u64;

// ---- the union-find, over LDS (workgroup scope) or global memory (agent scope)

enum { kFrLds = 0, kFrAgent = 1, kFrQuiet = 2 };  // where a walk loads from; kFrQuiet: a forest nobody writes any more

template <int kMem>
__device__ __forceinline__ int fr_load(const int* p) {
  if (kMem == kFrLds) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (kMem == kFrAgent) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}

// the root of i's tree; *over is set when `bound` steps did not reach it
template <int kMem>
__device__ __forceinline__ int fr_find(const int* parent, int i, int bound, bool* over) {
  int r = i;
  for (int it = 0; it < bound; it++) {
    const int p = fr_load<kMem>(parent + r);
    if (p == r) return r;
    r = p;  // (p < r: the walk descends)
  }
  *over = true;
  return r;
}

template <int kMem>
__device__ __forceinline__ void fr_unite(int* parent, int a, int b, int bound, bool* over) {
  for (int it = 0; it < bound; it++) {
    a = fr_find<kMem>(parent, a, bound, over);
    b = fr_find<kMem>(parent, b, bound, over);
    if (a == b || *over) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(parent + a, b);
    if (old == a) return;  // a was still a root: linked
    a = old;               // another lane moved it: min(old, b) stands there now, and (old, b) is left to unite
  }
  *over = true;
}

// grid: tiles_x tiles_y workgroups. cost, pot: null without their test
__global__ void __launch_bounds__(kFrBlock) k_fr_tile(const int8_t* __restrict__ grid, const uint8_t* __restrict__ cost,
                                                      const unsigned* __restrict__ pot, int nx, int ny, int tiles_x,
                                                      int cost_max, int* __restrict__ parent, u64* __restrict__ sum) {
  __shared__ int8_t s_g[kFrPitch * kFrPitch];
  __shared__ int s_par[kFrTile * kFrTile];
  const int tile = blockIdx.x;
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int x0 = tx * kFrTile, y0 = ty * kFrTile;
  const int w = min(kFrTile, nx - x0), h = min(kFrTile, ny - y0);  // the tile's own cells
  for (int j = threadIdx.x; j < kFrPitch * kFrPitch; j += kFrBlock) {
    const int gx = x0 - 1 + j % kFrPitch, gy = y0 - 1 + j / kFrPitch;
    const bool in = gx >= 0 && gx < nx && gy >= 0 && gy < ny;
    s_g[j] = in ? grid[(size_t)gy * nx + gx] : (int8_t)VG_OCC_OCCUPIED;  // (outside the grid is not unknown)
  }
  __syncthreads();
  const int lx = threadIdx.x & (kFrTile - 1), r0 = (threadIdx.x / kFrTile) * kFrRows;
  const int rows = lx < w ? min(kFrRows, h - r0) : 0;  // the thread's cells inside the grid (<= 0: none)
  u64 n_front = 0, n_free = 0, n_unk = 0, n_rc = 0, n_ru = 0;
  for (int k = 0; k < kFrRows; k++) {
    const int ly = r0 + k;
    bool front = false;
    if (k < rows) {
      const int c = (ly + 1) * kFrPitch + lx + 1;
      const int8_t v = s_g[c];
      n_free += v == VG_OCC_FREE;
      n_unk += v == VG_OCC_UNKNOWN;
      if (v == VG_OCC_FREE && (s_g[c - kFrPitch] == VG_OCC_UNKNOWN || s_g[c + kFrPitch] == VG_OCC_UNKNOWN ||
                               s_g[c - 1] == VG_OCC_UNKNOWN || s_g[c + 1] == VG_OCC_UNKNOWN)) {
        const size_t g = (size_t)(y0 + ly) * nx + x0 + lx;
        if (cost && (int)cost[g] >= cost_max) n_rc++;
        else if (pot && pot[g] == kFrUnreached) n_ru++;
        else front = true;
      }
    }
    n_front += front;
    s_par[ly * kFrTile + lx] = front ? ly * kFrTile + lx : -1;
  }
  __syncthreads();
  bool over = false;
  for (int k = 0; k < rows; k++) {
    const int ly = r0 + k, c = ly * kFrTile + lx;
    if (s_par[c] < 0) continue;  // (whether a cell is a frontier cell does not change: a plain read will do)
    if (lx > 0 && s_par[c - 1] >= 0) fr_unite<kFrLds>(s_par, c, c - 1, kFrTile * kFrTile, &over);
    if (ly > 0) {
      if (lx > 0 && s_par[c - kFrTile - 1] >= 0) fr_unite<kFrLds>(s_par, c, c - kFrTile - 1, kFrTile * kFrTile, &over);
      if (s_par[c - kFrTile] >= 0) fr_unite<kFrLds>(s_par, c, c - kFrTile, kFrTile * kFrTile, &over);
      if (lx < kFrTile - 1 && s_par[c - kFrTile + 1] >= 0)
        fr_unite<kFrLds>(s_par, c, c - kFrTile + 1, kFrTile * kFrTile, &over);
    }
  }
  __syncthreads();
  for (int k = 0; k < rows; k++) {
    const int ly = r0 + k, c = ly * kFrTile + lx;
    int p = -1;
    if (s_par[c] >= 0) {
      const int r = fr_find<kFrLds>(s_par, c, kFrTile * kFrTile, &over);
      p = (y0 + r / kFrTile) * nx + x0 + r % kFrTile;
    }
    parent[(size_t)(y0 + ly) * nx + x0 + lx] = p;
  }
  n_front = wave_sum(n_front);
  n_free = wave_sum(n_free);
  n_unk = wave_sum(n_unk);
  n_rc = wave_sum(n_rc);
  n_ru = wave_sum(n_ru);
  if ((threadIdx.x & 63) == 0) {
    if (n_front) atomicAdd(&sum[kFrCells], n_front);
    if (n_free) atomicAdd(&sum[kFrFree], n_free);
    if (n_unk) atomicAdd(&sum[kFrUnknown], n_unk);
    if (n_rc) atomicAdd(&sum[kFrRejCost], n_rc);
    if (n_ru) atomicAdd(&sum[kFrRejUnreached], n_ru);
  }
  if (over) atomicOr(&sum[kFrFlag], 1ull);
}

// lanes: n_v = (tiles_x - 1) ny cells with ix % kFrTile == 0, ix > 0, then n_h = (tiles_y - 1) nx cells with
// iy % kFrTile == 0, iy > 0 (a cell with both is named twice: once for each rim)
__global__ void __launch_bounds__(kFrBlock) k_fr_merge(int* parent, int nx, int ny, long long n_v, long long n_h,
                                                       u64* __restrict__ sum) {
  long long j = (long long)blockIdx.x * kFrBlock + threadIdx.x;
  int x, y, qx[3], qy[3];
  if (j < n_v) {
    x = (int)(j / ny + 1) * kFrTile, y = (int)(j % ny);
    for (int k = 0; k < 3; k++) qx[k] = x - 1, qy[k] = y - 1 + k;
  } else if ((j -= n_v) < n_h) {
    x = (int)(j % nx), y = (int)(j / nx + 1) * kFrTile;
    for (int k = 0; k < 3; k++) qx[k] = x - 1 + k, qy[k] = y - 1;
    if (x > 0 && x % kFrTile == 0) qx[0] = -1;  // (the corner's diagonal: the other rim's lane of this cell has it)
  } else {
    return;
  }
  const int i = y * nx + x;
  if (parent[i] < 0) return;  // (whether a cell is a frontier cell does not change here: a plain read will do)
  const int bound = nx * ny;
  bool over = false;
  for (int k = 0; k < 3; k++) {
    if (qx[k] < 0 || qx[k] >= nx || qy[k] < 0 || qy[k] >= ny) continue;
    const int n = qy[k] * nx + qx[k];
    if (parent[n] >= 0) fr_unite<kFrAgent>(parent, i, n, bound, &over);
  }
  if (over) atomicOr(&sum[kFrFlag], 1ull);
}

// the number of set flags among the workgroup's lanes, to every lane; *before: among the lanes before this one
__device__ __forceinline__ int fr_block_rank(bool flag, int* before) {
  __shared__ int s_w[kFrBlock / 64];
  const u64 m = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  __syncthreads();  // (a call before this one has read s_w)
  if (lane == 0) s_w[wave] = __popcll(m);
  __syncthreads();
  int base = 0, total = 0;
  for (int k = 0; k < kFrBlock / 64; k++) {
    if (k < wave) base += s_w[k];
    total += s_w[k];
  }
  *before = base + __popcll(m & ((1ull << lane) - 1ull));
  return total;
}

// one lane per cell. parent: read only
__global__ void __launch_bounds__(kFrBlock) k_fr_flatten(const int* __restrict__ parent, int cells, int* __restrict__ label,
                                                         int* __restrict__ counts, u64* __restrict__ sum) {
  const int i = blockIdx.x * kFrBlock + threadIdx.x;
  bool over = false, root = false;
  if (i < cells) {
    const int p = parent[i];
    root = p == i;
    label[i] = p < 0 ? -1 : fr_find<kFrQuiet>(parent, p, cells, &over);
  }
  int before;
  const int total = fr_block_rank(root, &before);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
  if (over) atomicOr(&sum[kFrFlag], 1ull);
}

// one workgroup: counts[0 .. n) to their exclusive prefix sums in place, the total to sum[slot]
__global__ void __launch_bounds__(kFrBlock) k_fr_scan(int* __restrict__ counts, int n, u64* __restrict__ sum, int slot) {
  __shared__ int s_part[kFrBlock];
  const int per = (n + kFrBlock - 1) / kFrBlock;
  const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
  int t = 0;
  for (int k = lo; k < hi; k++) t += counts[k];
  s_part[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int k = 0; k < kFrBlock; k++) {
      const int v = s_part[k];
      s_part[k] = run;
      run += v;
    }
    sum[slot] = (u64)run;
  }
  __syncthreads();
  int run = s_part[threadIdx.x];
  for (int k = lo; k < hi; k++) {
    const int v = counts[k];
    counts[k] = run;
    run += v;
  }
}

// one lane per cell: a root's dense id (counts: the workgroups' offsets), its record started, the id left in parent
__global__ void __launch_bounds__(kFrBlock) k_fr_number(int* __restrict__ parent, int cells, const int* __restrict__ counts,
                                                        vg_frontier_rec* __restrict__ rec) {
  const int i = blockIdx.x * kFrBlock + threadIdx.x;
  const bool root = i < cells && parent[i] == i;
  int before;
  fr_block_rank(root, &before);
  if (!root) return;
  const int id = counts[blockIdx.x] + before;
  vg_frontier_rec r;
  r.label = i, r.size = 0;
  r.x_min = r.y_min = INT_MAX, r.x_max = r.y_max = -1;
  r.sum_x = r.sum_y = 0;
  r.best_cell = -1, r.best_pot = 0xFFFFFFFFu;  // (as one 64-bit key: above every pot << 32 | cell)
  r.reserved[0] = r.reserved[1] = 0;
  rec[id] = r;
  parent[i] = id;
}

// one lane per cell; ids: parent after k_fr_number. kCombine: where all the frontier cells of a wave lie in one
// component the wave adds once: the variant in use, 5 to 10 % faster on mid-sized frontiers and 25 to 45 times where
// one frontier holds millions of cells; without it every lane adds for itself
template <bool kCombine>
__global__ void __launch_bounds__(kFrBlock) k_fr_stats(const int* __restrict__ label, const int* __restrict__ ids,
                                                       const unsigned* __restrict__ pot, int nx, int cells,
                                                       vg_frontier_rec* __restrict__ rec) {
  const int i = blockIdx.x * kFrBlock + threadIdx.x;
  const int l = i < cells ? label[i] : -1;
  const bool front = l >= 0;
  const int id = front ? ids[l] : -1;
  const int x = i % nx, y = i / nx;
  const u64 key = front && pot ? ((u64)pot[i] << 32 | (u64)(unsigned)i) : ~0ull;
  if (kCombine) {
    const u64 m = __ballot(front);
    if (!m) return;
    const int id0 = __shfl(id, __ffsll((unsigned long long)m) - 1, 64);
    if (!__ballot(front && id != id0)) {  // (wave-uniform)
      const int n = __popcll(m);
      const u64 sx = wave_sum(front ? (u64)x : 0ull), sy = wave_sum(front ? (u64)y : 0ull);
      const int x_lo = wave_min(front ? x : INT_MAX), y_lo = wave_min(front ? y : INT_MAX);
      const int x_hi = wave_max(front ? x : -1), y_hi = wave_max(front ? y : -1);
      const u64 best = wave_min(key);
      if ((threadIdx.x & 63) == 0) {
        vg_frontier_rec* r = rec + id0;
        atomicAdd(&r->size, n);
        atomicMin(&r->x_min, x_lo), atomicMin(&r->y_min, y_lo);
        atomicMax(&r->x_max, x_hi), atomicMax(&r->y_max, y_hi);
        atomicAdd(reinterpret_cast<u64*>(&r->sum_x), sx), atomicAdd(reinterpret_cast<u64*>(&r->sum_y), sy);
        if (pot) atomicMin(reinterpret_cast<u64*>(&r->best_cell), best);
      }
      return;
    }
  }
  if (!front) return;
  vg_frontier_rec* r = rec + id;
  atomicAdd(&r->size, 1);
  atomicMin(&r->x_min, x), atomicMin(&r->y_min, y);
  atomicMax(&r->x_max, x), atomicMax(&r->y_max, y);
  atomicAdd(reinterpret_cast<u64*>(&r->sum_x), (u64)x), atomicAdd(reinterpret_cast<u64*>(&r->sum_y), (u64)y);
  if (pot) atomicMin(reinterpret_cast<u64*>(&r->best_cell), key);
}
static_assert(offsetof(vg_frontier_rec, best_cell) % 8 == 0 &&
                  offsetof(vg_frontier_rec, best_pot) == offsetof(vg_frontier_rec, best_cell) + 4,
              "best_cell and best_pot: one little-endian 64-bit key, pot << 32 | cell");

// one lane per component: per workgroup the records with size >= min_size; the largest size
__global__ void __launch_bounds__(kFrBlock) k_fr_keep(const vg_frontier_rec* __restrict__ rec, int n, int min_size,
                                                      int* __restrict__ counts, u64* __restrict__ sum) {
  const int id = blockIdx.x * kFrBlock + threadIdx.x;
  const int size = id < n ? rec[id].size : 0;
  int before;
  const int total = fr_block_rank(size >= min_size, &before);  // (min_size >= 1: a lane past n keeps nothing)
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
  const int big = wave_max(size);
  if ((threadIdx.x & 63) == 0 && big) atomicMax(&sum[kFrMaxSize], (u64)big);
}

// one lane per component: the kept records in order (counts: the workgroups' offsets), the first max_records of them
__global__ void __launch_bounds__(kFrBlock) k_fr_emit(const vg_frontier_rec* __restrict__ rec, int n, int min_size,
                                                      const int* __restrict__ counts, int max_records, bool has_best,
                                                      vg_frontier_rec* __restrict__ out) {
  const int id = blockIdx.x * kFrBlock + threadIdx.x;
  const bool keep = id < n && rec[id].size >= min_size;
  int before;
  fr_block_rank(keep, &before);
  const int at = counts[blockIdx.x] + before;
  if (!keep || at >= max_records) return;
  vg_frontier_rec r = rec[id];
  if (!has_best) r.best_cell = -1, r.best_pot = 0u;
  out[at] = r;
}

// ---- host side

static int fr_bufs(vg_ctx* ctx, size_t cells) {
  FrontierBufs& b = ctx->fr;
  VG_HIP(b.sum.reserve(kFrSlots));
  VG_HIP(b.counts.reserve(kFrMaxCounts + 1));
  VG_HIP(b.out.reserve(VG_FRONTIER_MAX_RECORDS));
  VG_HIP(b.grid.reserve(cells));
  VG_HIP(b.parent.reserve(cells));
  VG_HIP(b.label.reserve(cells));
  return VG_OK;
}

int frontiers_dev(vg_ctx* ctx, const int8_t* grid, const uint8_t* cost, const vg_frontier_params* prm, int32_t* labels,
                  vg_frontier_rec* recs, int max_records, vg_frontier_summary* out) {
  const int nx = prm->nx, ny = prm->ny;
  const size_t cells = (size_t)nx * (size_t)ny;
  const int tiles_x = (nx + kFrTile - 1) / kFrTile, tiles_y = (ny + kFrTile - 1) / kFrTile;
  const bool use_cost = prm->flags & 1, use_pot = prm->flags & 2;
  const int cost_max = prm->cost_max ? prm->cost_max : VG_COST_INSCRIBED;
  const int min_size = prm->min_size > 0 ? prm->min_size : 1;
  FrontierBufs& b = ctx->fr;
  VG_TRY(fr_bufs(ctx, cells));
  if (cost) VG_HIP(b.cost.reserve(cells));
  hipStream_t s = ctx->stream;
  const int8_t* d_grid;
  const uint8_t* d_cost;  // (null without the cost test; a host plane comes with use_cost only)
  const unsigned* d_pot = use_pot ? ctx->nav.pot.p : nullptr;
  u64 h_sum[kFrSlots];
  b.t.clear();
  VG_TRY(plane_in(ctx, grid, b.grid, ctx->occ.grid.p, cells, &d_grid));
  VG_TRY(plane_in(ctx, cost, b.cost, use_cost ? ctx->clr.cost.p : nullptr, cells, &d_cost));
  VG_HIP(hipMemsetAsync(b.sum, 0, kFrSlots * sizeof(u64), s));
  VG_HIP(b.t.begin(s));
  k_fr_tile<<<(unsigned)(tiles_x * tiles_y), kFrBlock, 0, s>>>(d_grid, d_cost, d_pot, nx, ny, tiles_x, cost_max, b.parent,
                                                                b.sum);
  VG_HIP(hipGetLastError());
  const long long n_v = (long long)(tiles_x - 1) * ny, n_h = (long long)(tiles_y - 1) * nx;
  const long long rim = n_v + n_h > 0 ? n_v + n_h : 1;  // (a single tile: one workgroup that finds no lane)
  k_fr_merge<<<(unsigned)((rim + kFrBlock - 1) / kFrBlock), kFrBlock, 0, s>>>(b.parent, nx, ny, n_v, n_h, b.sum);
  VG_HIP(hipGetLastError());
  const unsigned blocks = (unsigned)((cells + kFrBlock - 1) / kFrBlock);
  k_fr_flatten<<<blocks, kFrBlock, 0, s>>>(b.parent, (int)cells, b.label, b.counts, b.sum);
  k_fr_scan<<<1, kFrBlock, 0, s>>>(b.counts, (int)blocks, b.sum, kFrComponents);
  VG_HIP(hipGetLastError());
  // the number of components sizes the records, and the forest is final: the bound's flag is too
  VG_HIP(hipMemcpyAsync(h_sum, b.sum, sizeof(h_sum), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  if (h_sum[kFrFlag]) {
    ctx->err = "vg_frontiers: a walk up the union-find forest did not end within nx ny steps";
    return VG_E_CAPACITY;
  }
  const int n_comp = (int)h_sum[kFrComponents];
  VG_HIP(b.rec.reserve_pow2((size_t)n_comp));
  k_fr_number<<<blocks, kFrBlock, 0, s>>>(b.parent, (int)cells, b.counts, b.rec);
  VG_HIP(hipGetLastError());
  if (b.combine) k_fr_stats<true><<<blocks, kFrBlock, 0, s>>>(b.label, b.parent, d_pot, nx, (int)cells, b.rec);
  else k_fr_stats<false><<<blocks, kFrBlock, 0, s>>>(b.label, b.parent, d_pot, nx, (int)cells, b.rec);
  VG_HIP(hipGetLastError());
  const unsigned rblocks = n_comp > 0 ? (unsigned)((n_comp + kFrBlock - 1) / kFrBlock) : 1u;  // (none: one idle workgroup)
  k_fr_keep<<<rblocks, kFrBlock, 0, s>>>(b.rec, n_comp, min_size, b.counts, b.sum);
  k_fr_scan<<<1, kFrBlock, 0, s>>>(b.counts, (int)rblocks, b.sum, kFrKept);
  k_fr_emit<<<rblocks, kFrBlock, 0, s>>>(b.rec, n_comp, min_size, b.counts, max_records, use_pot, b.out);
  VG_HIP(b.t.end(s));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(h_sum, b.sum, sizeof(h_sum), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  VG_HIP(b.t.collect());
  const long long n_kept = (long long)h_sum[kFrKept];
  h_sum[kFrWritten] = (u64)(n_kept < max_records ? n_kept : max_records);
  // (into the caller's arrays only once every kernel ran: a failed launch writes nothing)
  if (labels) VG_HIP(hipMemcpyAsync(labels, b.label, cells * sizeof(int), hipMemcpyDeviceToHost, s));
  if (h_sum[kFrWritten])
    VG_HIP(hipMemcpyAsync(recs, b.out, (size_t)h_sum[kFrWritten] * sizeof(vg_frontier_rec), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  memcpy(out, h_sum, sizeof(vg_frontier_summary));
  return VG_OK;
}

}  // namespace vg

// Measurement hooks. vgx_frontier_ms: the device time of the last vg_frontiers call's kernels (HIP events on the
// context stream around them; the host's read of the component count in between is inside).
// vgx_frontier_combine: whether k_fr_stats combines the lanes of a wave that lie in one component (the default) or
// every lane adds for itself; the outputs are the same bytes either way
extern "C" int vgx_frontier_ms(vg_ctx* ctx, double* ms) {
  if (!ctx || !ms || !ctx->fr.t.armed()) return VG_E_ARG;
  *ms = ctx->fr.t.ms;
  return VG_OK;
}
extern "C" int vgx_frontier_combine(vg_ctx* ctx, int on) {
  if (!ctx) return VG_E_ARG;
  ctx->fr.combine = on != 0;
  return VG_OK;
}
