"""Numpy restatement of the navigation function's definition (vina_gpu.h
"Navigation function"): the traversal table, the saturated potential by
whole-plane relaxation sweeps to the fixed point in int64, the descent and the
summary; with them the case generators the tests share. test_nav_ref.py pins it
against scipy's Dijkstra on the same edge list without a device."""
import math

import numpy as np

SAT, UNREACHED = 0xFFFFFFFE, 0xFFFFFFFF      # VG_NAV_SAT, VG_NAV_UNREACHED
K_ORTHO, K_DIAG = 12, 17                     # VG_NAV_K_*
REACHED, NO_PATH, TRUNCATED, STUCK = 0, 1, 2, 3
LETHAL, INSCRIBED, NO_INFO = 254, 253, 255   # VG_COST_*
FAR = 1 << 62                                # "no path yet" inside the sweeps
# (dx, dy) of the 8 neighbours in ascending linear index
NEIGHBOURS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]
REPRODUCIBLE = ("n_goals_used", "n_goals_ignored", "cells_passable", "cells_reached", "cells_saturated", "max_pot")


def trav_table(flags=0, neutral=0, lethal_from=0, unknown_as=0, factor=0.0):
    """The default table: uint16 [256], 0 impassable; zeros take nav2's 50, 253, 0.8."""
    neutral, lethal_from, factor = neutral or 50, lethal_from or 253, factor or 0.8
    t = np.zeros(256, dtype=np.int64)
    for c in range(255):
        if c < lethal_from:
            t[c] = neutral + int(math.floor(factor * c))
    if flags & 1:
        t[255] = t[unknown_as]
    assert t.max() <= 65535
    return t.astype(np.uint16)


def used_goals(cost, trav, goals):
    """The goals inside the grid on a passable cell, (n, 2) of ix, iy, and the number ignored."""
    ny, nx = cost.shape
    g = np.asarray(goals, dtype=np.int64).reshape(-1, 2)
    ok = (g[:, 0] >= 0) & (g[:, 0] < nx) & (g[:, 1] >= 0) & (g[:, 1] < ny)
    ok[ok] = trav[cost[g[ok, 1], g[ok, 0]]] > 0
    return g[ok], int((~ok).sum())


def _padded(cost, trav):
    """The price plane int64 [ny + 2, nx + 2] with an impassable rim."""
    t = np.zeros((cost.shape[0] + 2, cost.shape[1] + 2), dtype=np.int64)
    t[1:-1, 1:-1] = np.asarray(trav, dtype=np.int64)[cost]
    return t


def potential(cost, trav, goals):
    """pot uint32 [ny, nx]: every sweep relaxes every cell against its 8 neighbours of the sweep before, with
    saturation at SAT, until a sweep changes nothing."""
    cost = np.asarray(cost, dtype=np.uint8)
    ny, nx = cost.shape
    t = _padded(cost, trav)
    ok = t > 0
    p = np.full(t.shape, FAR, dtype=np.int64)
    g, _ = used_goals(cost, trav, goals)
    p[g[:, 1] + 1, g[:, 0] + 1] = 0
    core = (slice(1, ny + 1), slice(1, nx + 1))
    steps = []
    for dx, dy in NEIGHBOURS:
        nb = (slice(1 + dy, ny + 1 + dy), slice(1 + dx, nx + 1 + dx))
        edge = ok[core] & ok[nb]
        if dx and dy:   # no corner cutting: (ay, bx) and (by, ax)
            edge &= ok[1:ny + 1, 1 + dx:nx + 1 + dx] & ok[1 + dy:ny + 1 + dy, 1:nx + 1]
        w = (K_DIAG if dx and dy else K_ORTHO) * (t[core] + t[nb])
        steps.append((nb, edge, w))
    while True:
        best = p[core].copy()
        for nb, edge, w in steps:
            q = p[nb]
            cand = np.where(edge & (q < FAR), np.minimum(q + w, SAT), FAR)
            np.minimum(best, cand, out=best)
        if np.array_equal(best, p[core]):
            break
        p[core] = best
    return np.where(p[core] >= FAR, UNREACHED, p[core]).astype(np.uint32)


def edge_weight(cost, trav, a, b):
    """w(a, b) of two cells (ix, iy) a king's move apart, or None where the graph has no such edge."""
    ny, nx = cost.shape
    (ax, ay), (bx, by) = a, b
    if not (0 <= bx < nx and 0 <= by < ny):
        return None
    ta, tb = int(trav[cost[ay, ax]]), int(trav[cost[by, bx]])
    if not ta or not tb:
        return None
    if ax != bx and ay != by and (not trav[cost[ay, bx]] or not trav[cost[by, ax]]):
        return None
    return (K_DIAG if ax != bx and ay != by else K_ORTHO) * (ta + tb)


def descend(cost, trav, pot, starts, max_len):
    """(cells int32 [S, max_len] (-1 past the end), len, status, path_cost) of the walks down pot."""
    cost = np.asarray(cost, dtype=np.uint8)
    ny, nx = cost.shape
    st = np.asarray(starts, dtype=np.int64).reshape(-1, 2)
    cells = np.full((st.shape[0], max_len), -1, dtype=np.int32)
    ln = np.zeros(st.shape[0], dtype=np.int32)
    status = np.full(st.shape[0], NO_PATH, dtype=np.int32)
    pc = np.full(st.shape[0], -1, dtype=np.int64)
    for s, (x, y) in enumerate(st.tolist()):
        if not (0 <= x < nx and 0 <= y < ny) or not trav[cost[y, x]] or pot[y, x] == UNREACHED:
            continue
        pc[s] = int(pot[y, x])
        status[s] = TRUNCATED
        for k in range(max_len):
            cells[s, k] = y * nx + x
            ln[s] = k + 1
            here = int(pot[y, x])
            if here == 0:
                status[s] = REACHED
                break
            best = None
            for dx, dy in NEIGHBOURS:
                w = edge_weight(cost, trav, (x, y), (x + dx, y + dy))
                if w is None or int(pot[y + dy, x + dx]) >= here:
                    continue
                key = int(pot[y + dy, x + dx]) + w
                if best is None or key < best[0]:
                    best = (key, x + dx, y + dy)
            if best is None:
                status[s] = STUCK
                break
            _, x, y = best
    return cells, ln, status, pc


def summary(cost, trav, goals, pot):
    """vg_nav_summary's reproducible fields as a dict, counted from the arrays."""
    cost = np.asarray(cost, dtype=np.uint8)
    g, ignored = used_goals(cost, trav, goals)
    reached = pot != UNREACHED
    return dict(n_goals_used=int(g.shape[0]), n_goals_ignored=ignored,
                cells_passable=int((np.asarray(trav)[cost] > 0).sum()), cells_reached=int(reached.sum()),
                cells_saturated=int((pot == SAT).sum()), max_pot=int(pot[reached].max()) if reached.any() else 0)


def check_paths(cost, trav, pot, cells, ln, status):
    """Asserts what holds along every path: consecutive cells are joined by an edge and pot strictly falls; a
    REACHED path ends on a goal; returns the number of steps checked."""
    nx = cost.shape[1]
    n = 0
    for s in range(cells.shape[0]):
        c = cells[s, :ln[s]].astype(np.int64)
        assert (cells[s, ln[s]:] == -1).all()
        for a, b in zip(c[:-1].tolist(), c[1:].tolist()):
            assert max(abs(a % nx - b % nx), abs(a // nx - b // nx)) == 1
            assert edge_weight(cost, trav, (a % nx, a // nx), (b % nx, b // nx)) is not None
            assert pot[b // nx, b % nx] < pot[a // nx, a % nx]
            n += 1
        if status[s] == REACHED:
            assert pot[c[-1] // nx, c[-1] % nx] == 0
    return n


# ---- case generators

def random_plane(nx, ny, seed, p_lethal=0.25, p_unknown=0.05):
    """uint8 [ny, nx]: costs 0 .. 252, about p_lethal of the cells 254 or 253, about p_unknown 255."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 253, size=(ny, nx)).astype(np.uint8)
    u = rng.random((ny, nx))
    c[u < p_lethal] = LETHAL
    c[u < 0.2 * p_lethal] = INSCRIBED
    c[(u >= p_lethal) & (u < p_lethal + p_unknown)] = NO_INFO
    return c


def passable_cells(cost, trav, n, seed):
    """n distinct passable cells (ix, iy), drawn with the seed."""
    iy, ix = np.nonzero(np.asarray(trav)[cost] > 0)
    pick = np.random.default_rng(seed).choice(ix.size, size=n, replace=False)
    return np.stack([ix[pick], iy[pick]], axis=1).astype(np.int32)


def serpentine(nx=200, ny=65):
    """Free rows and lethal walls on the odd rows, each wall open at one end, the ends alternating from the
    right: one corridor that runs through every free row. From (0, 0) to the far end of the last row it is
    ((ny + 1) / 2) (nx - 1) + (ny - 1) orthogonal steps."""
    c = np.zeros((ny, nx), dtype=np.uint8)
    c[1::2] = LETHAL
    for k, iy in enumerate(range(1, ny, 2)):
        c[iy, nx - 1 if k % 2 == 0 else 0] = 0
    return c
