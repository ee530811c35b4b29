// navfn.hip — the navigation function over the costmap and the paths down it
// (vg_navfn, vg_nav_paths; vina_gpu.h "Navigation function"): the minimum
// cost-to-go from every cell to the nearest goal, relaxed block-wise to its fixed
// point (the fast iterative scheme), in saturating 32-bit integers throughout.
//
// k_nav_init: one lane per cell looks the cell's price up (trav, 0 impassable)
// and counts the passable cells; the first n_goals lanes each set one goal's
// potential to 0 and wake its tile and, for a goal on the tile's rim, the tiles
// that hold the cell in their halo. The field was filled with kNavUnreached before
// the launch.
//
// k_nav_relax: one 256-thread workgroup per tile of kNavTile x kNavTile cells. A
// tile that nobody woke exits at once. An active one stages its cells' potentials
// and prices with a one-cell halo in LDS (66 x 66 x 6 bytes, 26 KB), relaxes every
// cell of its interior against its 8 neighbours in place, sweep after sweep, until
// a __syncthreads_or says that a whole sweep lowered nothing, and writes back the
// cells of its own that fell. A thread owns 16 consecutive cells of a column (the
// lanes of a wave: 64 consecutive cells of a row, LDS reads without conflicts) and
// walks them down in even sweeps and up in odd ones, so that a value crosses the
// thread's run in one sweep. If a cell on the tile's rim fell, the up to 8 tiles
// that hold it in their halo are woken in the next round's activity plane and the
// round's counter is bumped; the host launches rounds until one wakes nothing.
//
// Why this is safe and exact: a tile writes only cells it owns; every value ever
// held is the saturated length of a real walk to a goal (or kNavUnreached), so it
// never undercuts the answer; values only fall; aligned 32-bit loads and stores do
// not tear. A halo read that misses a neighbour's newer value merely leaves work
// to the next round, for which that neighbour has woken this tile. At the end no
// tile is awake, so no relaxation anywhere lowers anything, and that fixed point is
// min(D, kNavSat) whatever the order of events. No float, no atomic
// on the field; no workgroup waits for another; every device loop is bounded by a
// tile or grid dimension or by max_len.
//
// k_nav_sum: the summary's counts of the finished field, one atomic per wave and
// count. k_nav_descend: one lane per start walks down the field, the 8 neighbours'
// loads of a step issued together.
#include "vg_query.h"
#include "vg_reduce.h"

namespace vg {

constexpr int kNavBlock = 256;
constexpr int kNavTile = 64;                       // a tile's side, cells
constexpr int kNavPitch = kNavTile + 2;            // ... with its halo
constexpr int kNavRows = kNavTile * kNavTile / kNavBlock;  // cells of a column that a thread owns
constexpr int kNavBatchMax = 32;                   // rounds launched per read of their counters, at most
constexpr int kNavMaxPoints = VG_NAV_MAX_POINTS;
constexpr unsigned kNavSat = VG_NAV_SAT, kNavUnreached = VG_NAV_UNREACHED;
static_assert(kNavBlock == 4 * kNavTile && kNavRows == 16, "a thread's run of cells: one column of a quarter tile");

// the summary's int64 slots as the kernels index them (vg_nav_summary's order)
enum { kNavUsed = 0, kNavIgnored, kNavPassable, kNavReached, kNavSaturated, kNavMaxPot, kNavRounds, kNavTileRuns };

// p + w, saturating at kNavSat (p <= kNavSat, w < 2^22)
__device__ __forceinline__ unsigned nav_add(unsigned p, unsigned w) {
  const unsigned s = p + w;
  return (s < p || s > kNavSat) ? kNavSat : s;
}

// lanes: max(cells, n_goals)
__global__ void __launch_bounds__(kNavBlock) k_nav_init(const uint8_t* __restrict__ cost,
                                                        const uint16_t* __restrict__ table, int nx, int ny,
                                                        const int* __restrict__ goals, int n_goals,
                                                        uint16_t* __restrict__ trav, unsigned* __restrict__ pot,
                                                        int* __restrict__ act, int tiles_x,
                                                        unsigned long long* __restrict__ sum) {
  __shared__ uint16_t s_table[256];
  s_table[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const size_t cells = (size_t)nx * (size_t)ny;
  const size_t i = (size_t)blockIdx.x * kNavBlock + threadIdx.x;
  unsigned long long n_pass = 0, n_used = 0, n_ign = 0;
  if (i < cells) {
    const uint16_t t = s_table[cost[i]];
    trav[i] = t;
    n_pass = t != 0;
  }
  if (i < (size_t)n_goals) {
    const int gx = goals[2 * i], gy = goals[2 * i + 1];
    bool used = false;
    if (gx >= 0 && gx < nx && gy >= 0 && gy < ny) {
      const size_t c = (size_t)gy * nx + gx;
      if (s_table[cost[c]] != 0) {
        pot[c] = 0u;  // (several goals on one cell store the same value)
        // this store lowers the cell like any relaxation: wake its own tile and, where it lies on the tile's rim,
        // the tiles that hold it in their halo, i.e. the tiles of the 3 x 3 cells around it
        for (int dy = -1; dy <= 1; dy++)
          for (int dx = -1; dx <= 1; dx++) {
            const int ux = gx + dx, uy = gy + dy;
            if (ux >= 0 && ux < nx && uy >= 0 && uy < ny) act[(uy / kNavTile) * tiles_x + ux / kNavTile] = 1;
          }
        used = true;
      }
    }
    n_used = used, n_ign = !used;
  }
  n_pass = wave_sum(n_pass);
  n_used = wave_sum(n_used);
  n_ign = wave_sum(n_ign);
  if ((threadIdx.x & 63) == 0) {
    if (n_pass) atomicAdd(&sum[kNavPassable], n_pass);
    if (n_used) atomicAdd(&sum[kNavUsed], n_used);
    if (n_ign) atomicAdd(&sum[kNavIgnored], n_ign);
  }
}

// the 8 tiles around a tile, as bits of the rim mask: bit d is the tile at (dx, dy) = kNavDir[d]
__constant__ int8_t kNavDirX[8] = {0, 0, -1, 1, -1, 1, -1, 1};
__constant__ int8_t kNavDirY[8] = {-1, 1, 0, 0, -1, -1, 1, 1};

// grid: tiles_x tiles_y workgroups. act_cur: this round's activity plane (a tile clears its own entry);
// act_next: the next round's; marks: this round's count of tiles that woke another
__global__ void __launch_bounds__(kNavBlock) k_nav_relax(const uint16_t* __restrict__ trav, unsigned* pot, int nx,
                                                         int ny, int tiles_x, int tiles_y, int* act_cur,
                                                         int* act_next, unsigned* __restrict__ marks,
                                                         unsigned long long* __restrict__ sum) {
  __shared__ unsigned s_pot[kNavPitch * kNavPitch];
  __shared__ uint16_t s_tr[kNavPitch * kNavPitch];
  __shared__ int s_on, s_rim;
  const int tile = blockIdx.x;
  if (threadIdx.x == 0) {
    s_on = act_cur[tile];
    act_cur[tile] = 0;
    s_rim = 0;
  }
  __syncthreads();
  if (!s_on) return;
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int x0 = tx * kNavTile, y0 = ty * kNavTile;
  const int w = min(kNavTile, nx - x0), h = min(kNavTile, ny - y0);  // the tile's own cells
  for (int j = threadIdx.x; j < kNavPitch * kNavPitch; j += kNavBlock) {
    const int gx = x0 - 1 + j % kNavPitch, gy = y0 - 1 + j / kNavPitch;
    const bool in = gx >= 0 && gx < nx && gy >= 0 && gy < ny && gx <= x0 + w && gy <= y0 + h;
    const size_t g = (size_t)(in ? gy : 0) * nx + (in ? gx : 0);
    s_tr[j] = in ? trav[g] : (uint16_t)0;
    s_pot[j] = in ? pot[g] : kNavUnreached;
  }
  __syncthreads();
  const int lx = threadIdx.x & (kNavTile - 1), r0 = (threadIdx.x / kNavTile) * kNavRows;
  const int rows = lx < w ? min(kNavRows, h - r0) : 0;  // the thread's cells inside the grid (<= 0: none)
  unsigned fell = 0;  // bit j: the thread's cell r0 + j fell in this run
  int more = 0;  // the last sweep lowered something, in any thread
  for (int it = 0; it <= kNavTile * kNavTile; it++) {  // a sweep that lowers anything settles a cell for good
    int changed = 0;
    for (int k = 0; k < rows; k++) {
      const int j = (it & 1) ? rows - 1 - k : k;
      const int c = (r0 + j + 1) * kNavPitch + lx + 1;
      const unsigned tc = s_tr[c];
      if (!tc) continue;
      const unsigned tn = s_tr[c - kNavPitch], ts = s_tr[c + kNavPitch], tw = s_tr[c - 1], te = s_tr[c + 1];
      const unsigned tnw = s_tr[c - kNavPitch - 1], tne = s_tr[c - kNavPitch + 1];
      const unsigned tsw = s_tr[c + kNavPitch - 1], tse = s_tr[c + kNavPitch + 1];
      const unsigned pn = s_pot[c - kNavPitch], ps = s_pot[c + kNavPitch], pw = s_pot[c - 1], pe = s_pot[c + 1];
      const unsigned pnw = s_pot[c - kNavPitch - 1], pne = s_pot[c - kNavPitch + 1];
      const unsigned psw = s_pot[c + kNavPitch - 1], pse = s_pot[c + kNavPitch + 1];
      const unsigned cur = s_pot[c];
      unsigned best = cur;
      // (an impassable cell's potential is kNavUnreached for good, so an orthogonal step needs no look at its price)
      if (pn != kNavUnreached) best = min(best, nav_add(pn, VG_NAV_K_ORTHO * (tc + tn)));
      if (ps != kNavUnreached) best = min(best, nav_add(ps, VG_NAV_K_ORTHO * (tc + ts)));
      if (pw != kNavUnreached) best = min(best, nav_add(pw, VG_NAV_K_ORTHO * (tc + tw)));
      if (pe != kNavUnreached) best = min(best, nav_add(pe, VG_NAV_K_ORTHO * (tc + te)));
      if (pnw != kNavUnreached && tn && tw) best = min(best, nav_add(pnw, VG_NAV_K_DIAG * (tc + tnw)));
      if (pne != kNavUnreached && tn && te) best = min(best, nav_add(pne, VG_NAV_K_DIAG * (tc + tne)));
      if (psw != kNavUnreached && ts && tw) best = min(best, nav_add(psw, VG_NAV_K_DIAG * (tc + tsw)));
      if (pse != kNavUnreached && ts && te) best = min(best, nav_add(pse, VG_NAV_K_DIAG * (tc + tse)));
      if (best < cur) {
        s_pot[c] = best;
        fell |= 1u << j;
        changed = 1;
      }
    }
    more = __syncthreads_or(changed);
    if (!more) break;
  }
  int rim = 0;
  for (int j = 0; j < rows; j++)
    if (fell >> j & 1) {
      const int ly = r0 + j;
      pot[(size_t)(y0 + ly) * nx + x0 + lx] = s_pot[(ly + 1) * kNavPitch + lx + 1];
      const int n = ly == 0, s = ly == h - 1, we = lx == 0, e = lx == w - 1;
      rim |= n | s << 1 | we << 2 | e << 3 | (n & we) << 4 | (n & e) << 5 | (s & we) << 6 | (s & e) << 7;
    }
  if (rim) atomicOr(&s_rim, rim);
  __syncthreads();
  int woke = 0;
  if (threadIdx.x < 8 && (s_rim >> threadIdx.x & 1)) {
    const int ux = tx + kNavDirX[threadIdx.x], uy = ty + kNavDirY[threadIdx.x];
    if (ux >= 0 && ux < tiles_x && uy >= 0 && uy < tiles_y) act_next[uy * tiles_x + ux] = 1, woke = 1;
  }
  if (threadIdx.x == 0 && more) act_next[tile] = 1, woke = 1;  // (the sweep bound cut the run short: go on next round)
  woke = __syncthreads_or(woke);
  if (threadIdx.x == 0) {
    if (woke) atomicAdd(marks, 1u);
    atomicAdd(&sum[kNavTileRuns], 1ull);
  }
}

// grid-stride over the cells
__global__ void __launch_bounds__(kNavBlock) k_nav_sum(const unsigned* __restrict__ pot, size_t cells,
                                                       unsigned long long* __restrict__ sum) {
  unsigned long long n_reached = 0, n_sat = 0, p_max = 0;
  for (size_t i = (size_t)blockIdx.x * kNavBlock + threadIdx.x; i < cells; i += (size_t)gridDim.x * kNavBlock) {
    const unsigned p = pot[i];
    n_reached += p != kNavUnreached;
    n_sat += p == kNavSat;
    if (p != kNavUnreached && p > p_max) p_max = p;
  }
  n_reached = wave_sum(n_reached);
  n_sat = wave_sum(n_sat);
  p_max = wave_max(p_max);
  if ((threadIdx.x & 63) == 0) {
    if (n_reached) atomicAdd(&sum[kNavReached], n_reached);
    if (n_sat) atomicAdd(&sum[kNavSaturated], n_sat);
    if (p_max) atomicMax(&sum[kNavMaxPot], p_max);
  }
}

// one lane per start; cells: n_starts rows of max_len, filled with -1 before the launch
__global__ void __launch_bounds__(kNavBlock) k_nav_descend(const uint16_t* __restrict__ trav,
                                                           const unsigned* __restrict__ pot, int nx, int ny,
                                                           const int* __restrict__ starts, int n_starts, int max_len,
                                                           int* __restrict__ cells, int* __restrict__ len,
                                                           int* __restrict__ status, long long* __restrict__ path_cost) {
  const int s = blockIdx.x * kNavBlock + threadIdx.x;
  if (s >= n_starts) return;
  int x = starts[2 * s], y = starts[2 * s + 1];
  int* row = cells + (size_t)s * max_len;
  int n = 0, st = VG_NAV_NO_PATH;
  long long pc0 = -1;
  if (x >= 0 && x < nx && y >= 0 && y < ny && trav[(size_t)y * nx + x] != 0 && pot[(size_t)y * nx + x] != kNavUnreached) {
    unsigned pc = pot[(size_t)y * nx + x];
    pc0 = (long long)pc;
    st = VG_NAV_TRUNCATED;
    for (int k = 0; k < max_len; k++) {
      row[n++] = y * nx + x;
      if (pc == 0u) {
        st = VG_NAV_REACHED;
        break;
      }
      // the 3 x 3 block around (x, y), row by row: prices (0 outside the grid) and potentials, loaded together
      unsigned t[9], p[9];
#pragma unroll
      for (int q = 0; q < 9; q++) {
        const int ux = x + q % 3 - 1, uy = y + q / 3 - 1;
        const bool in = ux >= 0 && ux < nx && uy >= 0 && uy < ny;
        const size_t g = (size_t)(in ? uy : y) * nx + (in ? ux : x);
        const unsigned tv = trav[g], pv = pot[g];
        t[q] = in ? tv : 0u;
        p[q] = in ? pv : kNavUnreached;
      }
      unsigned long long best = ~0ull;
      int at = -1;
#pragma unroll
      for (int q = 0; q < 9; q++) {  // (ascending linear index, so < keeps the smallest among equals)
        if (q == 4) continue;
        const bool diag = (q & 1) == 0;
        // a diagonal step squeezes between the block's cells (row of q, column 1) and (row 1, column of q)
        const bool open = t[q] != 0u && (!diag || (t[q / 3 * 3 + 1] != 0u && t[3 + q % 3] != 0u));
        if (open && p[q] < pc) {
          const unsigned long long key =
              (unsigned long long)p[q] + (unsigned long long)((diag ? VG_NAV_K_DIAG : VG_NAV_K_ORTHO) * (t[4] + t[q]));
          if (key < best) best = key, at = q;
        }
      }
      if (at < 0) {
        st = VG_NAV_STUCK;
        break;
      }
      x += at % 3 - 1, y += at / 3 - 1;
      pc = p[at];
    }
  }
  len[s] = n;
  status[s] = st;
  path_cost[s] = pc0;
}

// ---- host side

static int nav_bufs(vg_ctx* ctx, size_t cells, size_t tiles) {
  NavBufs& b = ctx->nav;
  static_assert(sizeof(vg_nav_params) == 64 && sizeof(vg_nav_summary) == 128, "the records' documented sizes");
  VG_HIP(b.table.reserve(256));
  VG_HIP(b.goals.reserve(2 * (size_t)kNavMaxPoints));
  VG_HIP(b.marks.reserve(kNavBatchMax));
  VG_HIP(b.sum.reserve(1));
  VG_HIP(b.len.reserve(kNavMaxPoints));
  VG_HIP(b.status.reserve(kNavMaxPoints));
  VG_HIP(b.path_cost.reserve(kNavMaxPoints));
  VG_HIP(b.cost.reserve(cells));
  VG_HIP(b.trav.reserve(cells));
  VG_HIP(b.pot.reserve(cells));
  VG_HIP(b.act.reserve(2 * tiles));
  return VG_OK;
}

int navfn_dev(vg_ctx* ctx, const uint8_t* cost, const vg_nav_params* prm, const uint16_t* table, const int32_t* goals,
              int n_goals, uint32_t* pot, vg_nav_summary* out) {
  const int nx = prm->nx, ny = prm->ny;
  const size_t cells = (size_t)nx * (size_t)ny;
  const int tiles_x = (nx + kNavTile - 1) / kNavTile, tiles_y = (ny + kNavTile - 1) / kNavTile;
  const size_t tiles = (size_t)tiles_x * (size_t)tiles_y;
  NavBufs& b = ctx->nav;
  b.nx = b.ny = 0;  // (no field for vg_nav_paths until this call has finished)
  VG_TRY(nav_bufs(ctx, cells, tiles));
  hipStream_t s = ctx->stream;
  unsigned long long* d_sum = reinterpret_cast<unsigned long long*>(b.sum.p);
  const uint8_t* d_cost;
  int* act[2] = {b.act, b.act + tiles};
  b.t.clear();
  VG_HIP(hipMemcpyAsync(b.table, table, 256 * sizeof(uint16_t), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(b.goals, goals, 2 * (size_t)n_goals * sizeof(int), hipMemcpyHostToDevice, s));
  VG_TRY(plane_in(ctx, cost, b.cost, ctx->clr.cost.p, cells, &d_cost));
  VG_HIP(hipMemsetAsync(d_sum, 0, sizeof(vg_nav_summary), s));
  VG_HIP(hipMemsetAsync(b.act, 0, 2 * tiles * sizeof(int), s));
  VG_HIP(b.t.begin(s));
  VG_HIP(hipMemsetAsync(b.pot, 0xFF, cells * sizeof(unsigned), s));  // kNavUnreached everywhere
  const size_t lanes = cells > (size_t)n_goals ? cells : (size_t)n_goals;
  k_nav_init<<<(unsigned)((lanes + kNavBlock - 1) / kNavBlock), kNavBlock, 0, s>>>(d_cost, b.table, nx, ny, b.goals, n_goals,
                                                                                  b.trav, b.pot, act[0], tiles_x, d_sum);
  VG_HIP(hipGetLastError());
  // rounds in batches, each round with a counter of its own; a round that woke no tile ends the relaxation. Round r
  // reads act[r & 1] and fills act[~r & 1], which the round before left all clear
  const long long cap = (long long)cells + 2;
  long long rounds = 0;
  bool done = false;
  unsigned marks[kNavBatchMax];
  for (int batch = 4; !done; batch = batch < kNavBatchMax ? 2 * batch : batch) {
    if (rounds >= cap) {
      ctx->err = "vg_navfn: the relaxation did not reach its fixed point within nx ny + 2 rounds";
      return VG_E_CAPACITY;
    }
    const int n = (int)(cap - rounds < batch ? cap - rounds : batch);
    VG_HIP(hipMemsetAsync(b.marks, 0, kNavBatchMax * sizeof(unsigned), s));
    for (int r = 0; r < n; r++, rounds++)
      k_nav_relax<<<(unsigned)tiles, kNavBlock, 0, s>>>(b.trav, b.pot, nx, ny, tiles_x, tiles_y, act[rounds & 1],
                                                        act[~rounds & 1], b.marks + r, d_sum);
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(marks, b.marks, n * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    VG_HIP(hipStreamSynchronize(s));
    for (int r = 0; r < n; r++) done = done || marks[r] == 0;
  }
  const size_t blocks = (cells + kNavBlock - 1) / kNavBlock;
  k_nav_sum<<<(unsigned)(blocks < 2048 ? blocks : 2048), kNavBlock, 0, s>>>(b.pot, cells, d_sum);
  VG_HIP(b.t.end(s));
  VG_HIP(hipGetLastError());
  if (pot) VG_HIP(hipMemcpyAsync(pot, b.pot, cells * sizeof(unsigned), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(out, d_sum, sizeof(vg_nav_summary), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  out->rounds = rounds;
  VG_HIP(b.t.collect());
  b.nx = nx, b.ny = ny;
  return VG_OK;
}

int nav_paths_dev(vg_ctx* ctx, const int32_t* starts, int n_starts, int max_len, int32_t* cells, int32_t* len,
                  int32_t* status, int64_t* path_cost) {
  NavBufs& b = ctx->nav;
  hipStream_t s = ctx->stream;
  const size_t n_out = (size_t)n_starts * (size_t)max_len;
  VG_HIP(b.cells_out.reserve(n_out));
  b.t.clear();
  VG_HIP(hipMemcpyAsync(b.goals, starts, 2 * (size_t)n_starts * sizeof(int), hipMemcpyHostToDevice, s));
  VG_HIP(b.t.begin(s));
  VG_HIP(hipMemsetAsync(b.cells_out, 0xFF, n_out * sizeof(int), s));  // -1 past a path's end
  k_nav_descend<<<(n_starts + kNavBlock - 1) / kNavBlock, kNavBlock, 0, s>>>(b.trav, b.pot, b.nx, b.ny, b.goals, n_starts,
                                                                            max_len, b.cells_out, b.len, b.status,
                                                                            b.path_cost);
  VG_HIP(b.t.end(s));
  VG_HIP(hipGetLastError());
  // (into the caller's arrays only once the kernel ran: a failed launch writes nothing)
  VG_HIP(hipMemcpyAsync(cells, b.cells_out, n_out * sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(len, b.len, (size_t)n_starts * sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(status, b.status, (size_t)n_starts * sizeof(int), hipMemcpyDeviceToHost, s));
  if (path_cost)
    VG_HIP(hipMemcpyAsync(path_cost, b.path_cost, (size_t)n_starts * sizeof(long long), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  VG_HIP(b.t.collect());
  return VG_OK;
}

}  // namespace vg

// Measurement hook: the device time of the last vg_navfn or vg_nav_paths call's kernels (HIP events on the context
// stream around them; for vg_navfn the host's reads of the round counters in between are inside)
extern "C" int vgx_nav_ms(vg_ctx* ctx, double* ms) {
  if (!ctx || !ms || !ctx->nav.t.armed()) return VG_E_ARG;
  *ms = ctx->nav.t.ms;
  return VG_OK;
}
