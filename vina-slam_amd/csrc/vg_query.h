// vg_query.h — what the 2-D query layers (occupancy, terrain, clearance, navfn,
// frontiers, view gain) and localisability share on the host side of a call: the
// grid shape check, the opening, the state checks of the device planes a call may
// read, their upload, and the ray-cast grids' argument check and slab loop. A new
// query layer uses these and vg_reduce.h and does not write its own.
#pragma once
#include <cmath>

#include "vg_internal.h"

namespace vg {

// nx x ny is a legal grid: at least one cell, at most VG_OCC_MAX_CELLS, and no side above max_side (0: no side limit)
inline bool grid_shape_ok(int nx, int ny, int max_side) {
  if (nx < 1 || ny < 1 || (max_side && (nx > max_side || ny > max_side))) return false;
  return (long long)nx * (long long)ny <= (long long)VG_OCC_MAX_CELLS;
}

// query_host.cpp
// a query's opening: VG_E_STATE on a sharded context, then the drain of outstanding work. who: the entry point's name
int query_open(vg_ctx* ctx, const char* who);
// the device plane a call reads in place of an argument it left out (what: "grid == NULL", "cost == NULL", "flags bit
// 1") is there and nx x ny: the grid of the last vg_occupancy / vg_terrain, the cost plane of the last vg_clearance,
// the field of the last vg_navfn. Else VG_E_STATE, the text saying whether none was left or its shape differs
int held_grid_ok(vg_ctx* ctx, const char* who, const char* what, int nx, int ny);
int held_cost_ok(vg_ctx* ctx, const char* who, const char* what, int nx, int ny);
int held_field_ok(vg_ctx* ctx, const char* who, const char* what, int nx, int ny);

// *d: the device plane a query reads, the caller's host plane uploaded into the layer's own staging buffer (which
// the caller reserved for `cells`), or else `held`, the context's
template <class T>
inline int plane_in(vg_ctx* ctx, const T* host, DevBuf<T>& stage, const T* held, size_t cells, const T** d) {
  *d = host ? stage.p : held;
  if (host) VG_HIP(hipMemcpyAsync(stage, host, cells * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  return VG_OK;
}

// the arguments vg_occupancy and vg_terrain share (prm: either's parameters)
template <class Prm>
inline bool ray_grid_args_ok(const vg_ctx* ctx, const double* positions, int M, const double* dirs, int D,
                             const Prm* prm, const int8_t* grid, const void* out) {
  if (!ctx || !prm || !grid || !out || !dirs || M < 0 || (M > 0 && !positions)) return false;
  if (D < 1 || D > kInfoMaxDirs) return false;
  if (!(prm->res > 0.0) || !std::isfinite(prm->res) || !std::isfinite(prm->x0) || !std::isfinite(prm->y0)) return false;
  return grid_shape_ok(prm->nx, prm->ny, 0);
}

// the M origins of a ray-cast grid in slabs of kInfoSlab (slab D <= 2^24 lanes per launch): per slab the origins'
// upload into OccBufs::pos, then launch(m, n) for its m origins and n = m D rays between kt's events
template <class Launch>
inline int ray_slabs(vg_ctx* ctx, const double* positions, int M, int D, KernelTimer& kt, Launch launch) {
  OccBufs& b = ctx->occ;
  hipStream_t s = ctx->stream;
  for (int i0 = 0; i0 < M; i0 += kInfoSlab) {
    const int m = M - i0 < kInfoSlab ? M - i0 : kInfoSlab;
    VG_HIP(hipMemcpyAsync(b.pos, positions + 3 * (size_t)i0, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    VG_HIP(kt.begin(s));
    launch(m, m * D);
    VG_HIP(kt.end(s));
    VG_HIP(hipGetLastError());
    VG_HIP(hipStreamSynchronize(s));  // the slab's staging is reused by the next
    VG_HIP(kt.collect());
  }
  return VG_OK;
}

}  // namespace vg
