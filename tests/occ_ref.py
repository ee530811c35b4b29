"""Numpy restatement of the occupancy grid's definition (vina_gpu.h "Occupancy
grid") on top of ray ranges — raycast_ref.cast's for a brute-force reference,
or a device's own vg_raycast records.

Per ray the free segment is cut at every crossing t of a lattice line x = x0 +
k res (k = 0..nx) or y = y0 + k res (k = 0..ny); the crossings are sorted and
every piece of positive length marks the cell of its midpoint. Inside the grid
every cell wall is such a line, so a piece lies in one cell or wholly outside
the grid (dropped).

A ray is *uncertain* where rounding may put a mark into a neighbouring cell:
raycast_ref calls it grazing; two crossings, or a crossing and a segment end,
lie within EPS of each other (a lattice corner; a segment that starts or ends
on a line); the hit point or an end point of the free segment lies within EPS
of a lattice line; r d_z lies within EPS of a band limit."""
import numpy as np

import raycast_ref as rr

EPS = 1e-9   # metres


def _unit(dirs):
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _near_line(v, g0, res):
    """|v - the nearest lattice line g0 + k res| < EPS."""
    q = (v - g0) / res
    return np.abs(q - np.round(q)) * res < EPS


def _pieces(o, d, ta, tb, ok, x0, y0, res, nx, ny):
    """The pieces of the segments (ta, tb) of the rays `ok`: (ray index, ix, iy) of every piece inside the
    grid, one entry per ray and cell, and per ray whether two cuts (ends included) lie within EPS."""
    n = o.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = (x0 + res * np.arange(nx + 1)[None, :] - o[:, :1]) / d[:, :1]
        ty = (y0 + res * np.arange(ny + 1)[None, :] - o[:, 1:2]) / d[:, 1:2]
    T = np.concatenate([tx, ty], axis=1)
    T[~np.isfinite(T)] = np.inf
    a, b = ta[:, None], tb[:, None]
    close = ((np.abs(T - a) < EPS) | (np.abs(T - b) < EPS)).any(axis=1)
    S = np.sort(np.concatenate([np.where((T > a) & (T < b), T, np.inf), a, b], axis=1), axis=1)
    lo, hi = S[:, :-1], S[:, 1:]
    live = np.isfinite(hi) & np.isfinite(lo) & ok[:, None]
    with np.errstate(invalid="ignore"):
        close |= (live & (hi - lo < EPS)).any(axis=1)
        piece = live & (hi > lo)
    ri, pi = np.nonzero(piece)
    mid = 0.5 * (lo[ri, pi] + hi[ri, pi])
    ix = np.floor((o[ri, 0] + mid * d[ri, 0] - x0) / res).astype(np.int64)
    iy = np.floor((o[ri, 1] + mid * d[ri, 1] - y0) / res).astype(np.int64)
    ins = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
    key = np.unique(ri[ins] * (nx * ny) + iy[ins] * nx + ix[ins])
    ri, cell = key // (nx * ny), key % (nx * ny)
    return ri, cell % nx, cell // nx, close & ok


def marks(origins, dirs, r, x0, y0, res, nx, ny, z_lo=-0.3, z_hi=1.0, free_on_miss=0.0, t_min=0.0, ended=None,
          silent=None, near=None, chunk=2048):
    """origins (n, 3) or (3,), dirs (n, 3), r (n,): the hit's range, inf where the ray has none. ended:
    rays that mark nothing (truncated, left the key range, invalid); silent: rays that mark no free cell
    (flags bit 0 and VG_RAY_OCCUPIED); near: rays raycast_ref calls grazing. Returns (counts int32 [2, ny,
    nx]: n_free, n_occ; uncertain (n,) bool; in_band (n,) bool)."""
    d = _unit(dirs)
    n = d.shape[0]
    o = np.broadcast_to(np.asarray(origins, dtype=np.float64).reshape(-1, 3), d.shape)
    r = np.asarray(r, dtype=np.float64).reshape(n)
    ended = np.zeros(n, bool) if ended is None else np.asarray(ended, bool)
    silent = np.zeros(n, bool) if silent is None else np.asarray(silent, bool)
    unc = np.zeros(n, bool) if near is None else np.asarray(near, bool).copy()
    counts = np.zeros((2, ny, nx), dtype=np.int32)
    in_band_all = np.zeros(n, bool)
    for c0 in range(0, n, chunk):
        s = slice(c0, min(c0 + chunk, n))
        oo, dd, rr_ = o[s], d[s], r[s]
        hit = np.isfinite(rr_)
        valid = ~ended[s] & (hit | (free_on_miss > 0.0))
        r_end = np.where(hit, rr_, free_on_miss)
        dz = dd[:, 2]
        # the occupied mark
        rz = np.where(hit, rr_, 0.0) * dz
        in_band = hit & valid & (rz >= z_lo) & (rz <= z_hi)
        hp = oo + np.where(hit, rr_, 0.0)[:, None] * dd
        hx = np.floor((hp[:, 0] - x0) / res).astype(np.int64)
        hy = np.floor((hp[:, 1] - y0) / res).astype(np.int64)
        put = in_band & (hx >= 0) & (hx < nx) & (hy >= 0) & (hy < ny)
        np.add.at(counts[1], (hy[put], hx[put]), 1)
        u = hit & valid & ((np.abs(rz - z_lo) < EPS) | (np.abs(rz - z_hi) < EPS) | _near_line(hp[:, 0], x0, res)
                           | _near_line(hp[:, 1], y0, res))
        # the free segment
        with np.errstate(divide="ignore", invalid="ignore"):
            blo = np.where(dz > 0, z_lo / dz, np.where(dz < 0, z_hi / dz, -np.inf))
            bhi = np.where(dz > 0, z_hi / dz, np.where(dz < 0, z_lo / dz, np.inf))
        flat_out = (dz == 0) & (not z_lo <= 0.0 <= z_hi)
        ta = np.maximum(max(t_min, 0.0), blo)
        tb = np.minimum(r_end, bhi)
        ok = valid & ~silent[s] & ~flat_out & (ta < tb)
        ta, tb = np.where(ok, ta, 0.0), np.where(ok, tb, 1.0)
        ri, ix, iy, close = _pieces(oo, dd, ta, tb, ok, x0, y0, res, nx, ny)
        own = in_band[ri] & (ix == hx[ri]) & (iy == hy[ri])   # the in-band hit's own cell
        np.add.at(counts[0], (iy[~own], ix[~own]), 1)
        for t in (ta, tb):
            p = oo + t[:, None] * dd
            u |= ok & (_near_line(p[:, 0], x0, res) | _near_line(p[:, 1], y0, res))
        unc[s] |= u | close
        in_band_all[s] = in_band
    return counts, unc, in_band_all


def touched(origins, dirs, which, reach, x0, y0, res, nx, ny):
    """[ny, nx] bool: the cells within one cell of the whole ray (0, reach), band or hit aside, of the rays
    `which`: where an uncertain ray's marks may fall."""
    d = _unit(dirs)
    o = np.broadcast_to(np.asarray(origins, dtype=np.float64).reshape(-1, 3), d.shape)
    w = np.nonzero(np.asarray(which, bool))[0]
    m = np.zeros((ny + 2, nx + 2), bool)
    if w.size:
        _, ix, iy, _ = _pieces(o[w], d[w], np.zeros(w.size), np.full(w.size, float(reach)), np.ones(w.size, bool),
                               x0, y0, res, nx, ny)
        m[iy + 1, ix + 1] = True
    out = np.zeros((ny, nx), bool)
    for a in range(3):
        for b in range(3):
            out |= m[a:a + ny, b:b + nx]
    return out


def classify(counts, min_occ=1, min_free=1, occ_ratio=0.0):
    """int8 [ny, nx]: 100 / 0 / -1 by the header's rule."""
    f, o = counts[0].astype(np.int64), counts[1].astype(np.int64)
    occ = (o >= max(min_occ, 1)) & (o.astype(np.float64) >= max(occ_ratio, 0.0) * (o + f).astype(np.float64))
    g = np.where(occ, 100, np.where(f >= max(min_free, 1), 0, -1))
    return g.astype(np.int8)


def grid_ref(planes, positions, dirs, t_max=rr.T_MAX, t_min=0.0, **geom):
    """The definition from Context.map_planes() records: every position x every direction through
    raycast_ref.cast, then marks(). Returns (counts, uncertain (M D,), in_band, r (M D,), origins, dirs
    of the M D rays)."""
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    O, Dd = np.repeat(pos, d.shape[0], axis=0), np.tile(d, (pos.shape[0], 1))
    r, _, near = rr.cast(planes, O, Dd, t_min=t_min, t_max=t_max)
    counts, unc, in_band = marks(O, Dd, r, t_min=t_min, near=near, **geom)
    return counts, unc, in_band, r, O, Dd
