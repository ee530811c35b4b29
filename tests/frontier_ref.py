"""Numpy restatement of the exploration frontiers' definition (vina_gpu.h
"Exploration frontiers"): the frontier mask, the labels by plain flood fill in
ascending index (so a component's label is its smallest linear index), the
records, the summary and frontier_order; with them the case generators the tests
share. test_frontier_ref.py pins the labels against scipy.ndimage.label without
a device."""
import numpy as np

import nav_ref as nr

UNKNOWN, FREE, OCCUPIED = -1, 0, 100         # VG_OCC_*
UNREACHED = 0xFFFFFFFF                       # VG_NAV_UNREACHED
MAX_RECORDS = 65536                          # VG_FRONTIER_MAX_RECORDS
TILE = 64                                    # the kernels' tile side
REC = np.dtype([("label", "<i4"), ("size", "<i4"), ("x_min", "<i4"), ("y_min", "<i4"), ("x_max", "<i4"), ("y_max", "<i4"),
                ("sum_x", "<i8"), ("sum_y", "<i8"), ("best_cell", "<i4"), ("best_pot", "<u4"), ("reserved", "<i8", (2,))])
SUMMARY = ("n_frontier_cells", "n_components", "n_kept", "n_written", "max_size", "cells_free", "cells_unknown",
           "n_rejected_cost", "n_rejected_unreached")


def mask(grid, cost=None, pot=None, cost_max=0):
    """(frontier mask bool [ny, nx], n_rejected_cost, n_rejected_unreached). cost / pot: None without that test."""
    g = np.asarray(grid, dtype=np.int8)
    unk = np.zeros((g.shape[0] + 2, g.shape[1] + 2), dtype=bool)     # outside the grid is not unknown
    unk[1:-1, 1:-1] = g == UNKNOWN
    cand = (g == FREE) & (unk[:-2, 1:-1] | unk[2:, 1:-1] | unk[1:-1, :-2] | unk[1:-1, 2:])
    n_rc = n_ru = 0
    if cost is not None:
        rej = cand & (np.asarray(cost, dtype=np.uint8) >= (cost_max or 253))
        n_rc, cand = int(rej.sum()), cand & ~rej
    if pot is not None:
        rej = cand & (np.asarray(pot, dtype=np.uint32) == UNREACHED)
        n_ru, cand = int(rej.sum()), cand & ~rej
    return cand, n_rc, n_ru


def labels(m):
    """int32 [ny, nx]: the smallest linear index of the cell's 8-connected component of m, -1 off m."""
    ny, nx = m.shape
    lab = np.full((ny, nx), -1, dtype=np.int32)
    for i in np.flatnonzero(m.ravel()).tolist():                     # ascending: a fill starts at its component's minimum
        if lab.flat[i] >= 0:
            continue
        lab.flat[i] = i
        stack = [i]
        while stack:
            c = stack.pop()
            cx, cy = c % nx, c // nx
            for dx, dy in nr.NEIGHBOURS:
                x, y = cx + dx, cy + dy
                if 0 <= x < nx and 0 <= y < ny and m[y, x] and lab[y, x] < 0:
                    lab[y, x] = i
                    stack.append(y * nx + x)
    return lab


def records(lab, pot=None):
    """One REC per component of lab, in ascending label."""
    ny, nx = lab.shape
    roots = np.flatnonzero(lab.ravel() == np.arange(nx * ny))
    out = np.zeros(roots.size, dtype=REC)
    for k, r in enumerate(roots.tolist()):
        idx = np.flatnonzero(lab.ravel() == r)
        x, y = idx % nx, idx // nx
        out[k] = (r, idx.size, x.min(), y.min(), x.max(), y.max(), int(x.sum()), int(y.sum()), -1, 0, (0, 0))
        if pot is not None:
            p = np.asarray(pot, dtype=np.uint32).ravel()[idx]
            j = int(np.argmin(p))                                    # the first minimum: the smallest index among equals
            out[k]["best_cell"], out[k]["best_pot"] = idx[j], p[j]
    return out


def frontiers(grid, cost=None, pot=None, cost_max=0, min_size=0, max_records=4096):
    """(labels, the records kept and written, the summary as a dict) of vg_frontiers' definition."""
    g = np.asarray(grid, dtype=np.int8)
    m, n_rc, n_ru = mask(g, cost, pot, cost_max)
    lab = labels(m)
    rec = records(lab, pot)
    kept = rec[rec["size"] >= max(min_size, 1)]
    s = dict(n_frontier_cells=int(m.sum()), n_components=int(rec.size), n_kept=int(kept.size),
             n_written=int(min(kept.size, max_records)), max_size=int(rec["size"].max()) if rec.size else 0,
             cells_free=int((g == FREE).sum()), cells_unknown=int((g == UNKNOWN).sum()), n_rejected_cost=n_rc,
             n_rejected_unreached=n_ru)
    return lab, kept[:max_records], s


def frontier_order(recs):
    """The indices of recs by ascending (best_pot, label) when best_cell >= 0, otherwise by descending size, then
    ascending label (a plain sort of tuples)."""
    r = np.asarray(recs)
    if r.size and (r["best_cell"] >= 0).all():
        key = [(int(v["best_pot"]), int(v["label"])) for v in r]
    else:
        key = [(-int(v["size"]), int(v["label"])) for v in r]
    return np.array(sorted(range(len(key)), key=key.__getitem__), dtype=np.int64)


def spanning(lab):
    """The number of components of lab whose cells lie in more than one TILE x TILE tile."""
    ny, nx = lab.shape
    iy, ix = np.nonzero(lab >= 0)
    tile = (iy // TILE) * ((nx + TILE - 1) // TILE) + ix // TILE
    l = lab[iy, ix]
    return sum(1 for r in np.unique(l) if np.unique(tile[l == r]).size > 1)


# ---- case generators

def serpentine_grid(nx=200, ny=65):
    """nav_ref.serpentine()'s corridor made FREE and its walls UNKNOWN: every corridor cell touches a wall, so the
    whole corridor is one frontier."""
    return np.where(nr.serpentine(nx, ny) == 0, FREE, UNKNOWN).astype(np.int8)


def rooms(nx, ny, seed, n_blobs=None):
    """int8 [ny, nx]: free space with unknown discs of radius 2 .. 9 cells (about one per 600 cells) and a few
    occupied cells on their rims: mid-sized frontiers, one ring around each blob or cluster of blobs."""
    rng = np.random.default_rng(seed)
    g = np.zeros((ny, nx), dtype=np.int8)
    n = n_blobs if n_blobs is not None else max(1, nx * ny // 600)
    cx, cy, r = rng.integers(0, nx, n), rng.integers(0, ny, n), rng.integers(2, 10, n)
    yy, xx = np.mgrid[0:ny, 0:nx]
    for k in range(n):
        x0, x1, y0, y1 = max(cx[k] - r[k], 0), min(cx[k] + r[k] + 1, nx), max(cy[k] - r[k], 0), min(cy[k] + r[k] + 1, ny)
        sub = (xx[y0:y1, x0:x1] - cx[k]) ** 2 + (yy[y0:y1, x0:x1] - cy[k]) ** 2 <= r[k] ** 2
        g[y0:y1, x0:x1][sub] = UNKNOWN
    g.ravel()[rng.choice(nx * ny, size=max(1, nx * ny // 200), replace=False)] = OCCUPIED
    return g
