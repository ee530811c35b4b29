"""Numpy restatement of the view gain's definition (vina_gpu.h "View gain"): every
ray cell from the closed form (2 k a + n) div (2 n), the walk's tests in the
header's order, the visible set as a boolean window per viewpoint, the records,
the seen plane, the summary and view_order; with them the case generators the
tests share. All rays of a batch of viewpoints advance together, one numpy step
per k. test_view_ref.py pins it without a device by properties that do not come
from it."""
from fractions import Fraction

import numpy as np

UNKNOWN, FREE, OCCUPIED = -1, 0, 100         # VG_OCC_*
OK, OUTSIDE, BLOCKED = 0, 1, 2               # VG_VIEW_*
MAX_RADIUS = 255                             # VG_VIEW_MAX_RADIUS
REC = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("status", "<i4"), ("n_visible", "<i4"), ("n_unknown", "<i4"),
                ("n_free", "<i4"), ("n_occupied", "<i4"), ("n_rays_open", "<i4")])
SUMMARY = ("n_views", "n_ok", "n_outside", "n_blocked", "rays", "max_unknown_seen", "best_view", "cells_seen",
           "unknown_seen")
BATCH_CELLS = 1 << 23                        # window cells of one batch of viewpoints


def targets(R):
    """(8R, 2): every offset (dx, dy) with max(|dx|, |dy|) == R."""
    d = np.arange(-R, R + 1)
    dx, dy = np.meshgrid(d, d, indexing="xy")
    rim = np.maximum(np.abs(dx), np.abs(dy)) == R
    return np.stack([dx[rim], dy[rim]], axis=1).astype(np.int64)


def visible(grid, origins, R, max_unknown=0):
    """For origins (m, 2) that are inside the grid and not occupied: (vis bool [m, 2R+1, 2R+1], the window with
    vis[v, R + y - oy, R + x - ox] for the visible cell (x, y); rays open int [m]; rays ended by the diagonal rule)."""
    g = np.asarray(grid, dtype=np.int8)
    ny, nx = g.shape
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    m, W, n = o.shape[0], 2 * R + 1, R
    t = targets(R)
    ax, ay, sx, sy = np.abs(t[:, 0]), np.abs(t[:, 1]), np.sign(t[:, 0]), np.sign(t[:, 1])
    ox, oy = o[:, :1], o[:, 1:]
    vis = np.zeros((m, W, W), dtype=bool)
    vis[:, R, R] = True                                              # the origin's own cell
    alive = np.ones((m, t.shape[0]), dtype=bool)
    opened = np.ones_like(alive)                                     # False once a ray ended blocked
    u = np.zeros(alive.shape, dtype=np.int64)
    qx, qy = np.broadcast_to(ox, alive.shape), np.broadcast_to(oy, alive.shape)      # c_{k-1}
    vi = np.broadcast_to(np.arange(m)[:, None], alive.shape)
    n_diag = 0

    def at(x, y, where):
        """grid[y, x] where `where` (those lie inside the grid); FREE elsewhere."""
        v = np.zeros(where.shape, dtype=np.int8)
        v[where] = g[y[where], x[where]]
        return v

    for k in range(1, n + 1):
        px, py = (2 * k * ax + n) // (2 * n), (2 * k * ay + n) // (2 * n)
        cx, cy = ox + sx * px, oy + sy * py
        a = alive & (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)   # 1
        a &= (px * px + py * py <= R * R)[None, :]                  # 2
        diag = a & (cx != qx) & (cy != qy)                          # 3
        blocked = diag & (at(qx, cy, diag) == OCCUPIED) & (at(cx, qy, diag) == OCCUPIED)
        n_diag += int(blocked.sum())
        opened &= ~blocked
        a &= ~blocked
        vis[vi[a], (cy - oy + R)[a], (cx - ox + R)[a]] = True       # 4
        val = at(cx, cy, a)
        occ = a & (val == OCCUPIED)                                 # 5
        opened &= ~occ
        a &= ~occ
        unk = a & (val == UNKNOWN)                                  # 6
        u += unk
        if max_unknown > 0:
            a &= ~(unk & (u >= max_unknown))
        alive, qx, qy = a, cx, cy
    return vis, opened.sum(axis=1), n_diag


def view_gain(grid, views, radius, max_unknown=0):
    """(records REC [n], seen int32 [ny, nx], the summary as a dict, rays ended by the diagonal rule) of
    vg_view_gain's definition."""
    g = np.asarray(grid, dtype=np.int8)
    ny, nx = g.shape
    v = np.asarray(views, dtype=np.int64).reshape(-1, 2)
    R, W = int(radius), 2 * int(radius) + 1
    rec = np.zeros(v.shape[0], dtype=REC)
    rec["ix"], rec["iy"] = v[:, 0], v[:, 1]
    inside = (v[:, 0] >= 0) & (v[:, 0] < nx) & (v[:, 1] >= 0) & (v[:, 1] < ny)
    on_occ = np.zeros(v.shape[0], dtype=bool)
    on_occ[inside] = g[v[inside, 1], v[inside, 0]] == OCCUPIED
    rec["status"] = np.where(~inside, OUTSIDE, np.where(on_occ, BLOCKED, OK))
    seen = np.zeros((ny, nx), dtype=np.int32)
    ok = np.flatnonzero(rec["status"] == OK)
    n_diag = 0
    step = max(1, BATCH_CELLS // (W * W))
    for lo in range(0, ok.size, step):
        idx = ok[lo:lo + step]
        vis, n_open, nd = visible(g, v[idx], R, max_unknown)
        n_diag += nd
        mi, wy, wx = np.nonzero(vis)
        gx, gy = v[idx[mi], 0] + wx - R, v[idx[mi], 1] + wy - R      # (a visible cell lies inside the grid)
        val = g[gy, gx]
        count = lambda sel: np.bincount(mi[sel], minlength=idx.size)
        rec["n_unknown"][idx] = count(val == UNKNOWN)
        rec["n_occupied"][idx] = count(val == OCCUPIED)
        rec["n_free"][idx] = count((val != UNKNOWN) & (val != OCCUPIED))
        rec["n_visible"][idx] = np.bincount(mi, minlength=idx.size)
        rec["n_rays_open"][idx] = n_open
        np.add.at(seen, (gy, gx), 1)
    best = -1
    if ok.size:
        gain = rec["n_unknown"][ok]
        best = int(ok[gain == gain.max()][0])
    s = dict(n_views=int(v.shape[0]), n_ok=int(ok.size), n_outside=int((~inside).sum()), n_blocked=int(on_occ.sum()),
             rays=int(8 * R * ok.size), max_unknown_seen=int(rec["n_unknown"][best]) if best >= 0 else 0, best_view=best,
             cells_seen=int((seen > 0).sum()), unknown_seen=int(((seen > 0) & (g == UNKNOWN)).sum()))
    return rec, seen, s, n_diag


def view_order(recs, pots=None, min_gain=1):
    """The indices of the OK records with n_unknown >= min_gain: with pots by descending n_unknown / (pot + 1) as an
    exact fraction, then ascending pot, then index; without by descending n_unknown, then index."""
    r = np.asarray(recs)
    keep = [i for i in range(r.size) if r["status"][i] == OK and r["n_unknown"][i] >= min_gain]
    if pots is None:
        return np.array(sorted(keep, key=lambda i: (-int(r["n_unknown"][i]), i)), dtype=np.int64)
    p = [int(x) for x in np.asarray(pots).reshape(-1)]
    return np.array(sorted(keep, key=lambda i: (-Fraction(int(r["n_unknown"][i]), p[i] + 1), p[i], i)), dtype=np.int64)


def circle_count(R):
    """The number of integer (x, y) with x^2 + y^2 <= R^2."""
    d = np.arange(-R, R + 1)
    return int((d[:, None] ** 2 + d[None, :] ** 2 <= R * R).sum())


# ---- case generators

RING = 10                                    # the diamond ring's |x| + |y|
RING_ORIGINS = [(0, 0), (3, 2), (-5, 1), (0, -8), (-2, -6)]      # relative to its centre; all with |x| + |y| < RING


def diamond_ring(side=71):
    """(grid int8 [side, side], centre c): an 8-connected closed diamond of occupied cells |x - c| + |y - c| == RING,
    free inside, unknown outside."""
    c = side // 2
    d = np.abs(np.arange(side) - c)
    l1 = d[:, None] + d[None, :]
    return np.where(l1 == RING, OCCUPIED, np.where(l1 < RING, FREE, UNKNOWN)).astype(np.int8), c


def mixed_views(grid, n, seed):
    """(n, 2) int32 viewpoints of the grid: its four corners, cells outside it on every side, occupied cells, one
    cell twice, the rest drawn uniformly."""
    g = np.asarray(grid)
    ny, nx = g.shape
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (-1, 0), (0, -1), (nx, 3), (3, ny), (-40, -40),
             (nx + 300, ny + 300)]
    occ = np.argwhere(g == OCCUPIED)[:6, ::-1].tolist()
    rest = np.stack([rng.integers(0, nx, n), rng.integers(0, ny, n)], axis=1).tolist()
    v = (fixed + [tuple(c) for c in occ] + [tuple(c) for c in rest])[:n - 1]
    v.append(v[len(fixed) + len(occ)])                               # a cell named twice
    return np.array(v, dtype=np.int32)
