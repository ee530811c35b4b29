"""Numpy restatement of the terrain layer's definition (vina_gpu.h "Terrain
layer") on top of ray records — raycast_ref.cast's ranges with the planes'
normals for a brute-force reference, or a device's own vg_raycast records.

The pieces are occ_ref's: per ray the interval (max(t_min, 0), r_end) is cut at
every crossing of a lattice line, the crossings are sorted and every piece of
positive length belongs to the cell of its midpoint. Here they are kept in the
order of the walk, because the ground reference is carried along it.

A ray is *uncertain* where rounding may move a mark or flip a comparison:
occ_ref calls it uncertain (grazing, a lattice corner, an end or the hit on a
lattice line); a quantised height (the origin's reference, a piece's midpoint
inside the grid, the hit) has z / z_res within Q_EPS of an integer; |normal[2]|
lies within N_EPS of up_min; range d_z lies within occ_ref.EPS of g_lo or g_hi."""
import numpy as np

import occ_ref as oc

NONE = -2 ** 31
LIMIT = 2 ** 30
Q_EPS = 1e-6
N_EPS = 1e-9
UP_MIN = 0.8191520442889918   # cos 35 degrees


def q(z, z_res):
    """floor(z / z_res) in double as int64, held to +-2^30 (|q| = 2^30: out of range; NaN lands on -2^30)."""
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(np.asarray(z, dtype=np.float64) / z_res)
    c = np.where(c > -float(LIMIT), np.where(c < float(LIMIT), c, float(LIMIT)), -float(LIMIT))   # (NaN: the last branch)
    return c.astype(np.int64)


def _near_int(z, z_res):
    v = np.asarray(z, dtype=np.float64) / z_res
    return np.abs(v - np.round(v)) < Q_EPS


def defaults(x0, y0, res, nx, ny, free_on_miss=0.0, min_occ=0, min_free=0, occ_ratio=0.0, flags=0, min_ground=0,
             z_res=0.0, up_min=0.0, g_lo=0.0, g_hi=0.0, clear_lo=0.0, clear_hi=0.0, sensor_height=0.0, step_max=0.0,
             t_min=0.0):
    """vg_terrain_params with the defaults applied and clo, chi, smax quantised, as a dict."""
    z_res = z_res if z_res > 0.0 else 0.001
    if g_lo == 0.0 and g_hi == 0.0:
        g_lo, g_hi = -3.0, -0.1
    if clear_lo == 0.0 and clear_hi == 0.0:
        clear_lo, clear_hi = 0.15, 1.5
    return dict(x0=x0, y0=y0, res=res, nx=nx, ny=ny, free_on_miss=max(free_on_miss, 0.0), min_occ=max(min_occ, 1),
                min_free=max(min_free, 1), occ_ratio=max(occ_ratio, 0.0), flags=flags, min_ground=max(min_ground, 1),
                z_res=z_res, up_min=up_min if up_min > 0.0 else UP_MIN, g_lo=g_lo, g_hi=g_hi,
                clo=int(q(clear_lo, z_res)), chi=int(q(clear_hi, z_res)),
                smax=int(q(step_max, z_res)) if flags & 2 else 0, sensor_height=sensor_height, t_min=t_min)


def cells(g_n, g_sum, g_min, g_max, min_ground=1):
    """The per-cell stage on ground planes [ny, nx]: (elev int32, step int32, (cells_ground, max_step,
    max_spread)). Pure integer arithmetic (Python's // is the mathematical floor)."""
    g_n = np.asarray(g_n, dtype=np.int64)
    g_sum = np.asarray(g_sum, dtype=np.int64)
    ny, nx = g_n.shape
    has = g_n >= max(min_ground, 1)
    elev = np.where(has, g_sum // np.where(has, g_n, 1), NONE)
    pad = np.full((ny + 2, nx + 2), NONE, dtype=np.int64)
    pad[1:-1, 1:-1] = elev
    step = np.zeros((ny, nx), dtype=np.int64)
    for a in range(3):
        for b in range(3):
            if (a, b) == (1, 1):
                continue
            nb = pad[a:a + ny, b:b + nx]
            step = np.maximum(step, np.where(has & (nb != NONE), np.abs(elev - nb), 0))
    spread = np.where(g_n > 0, np.asarray(g_max, dtype=np.int64) - np.asarray(g_min, dtype=np.int64), 0)
    return elev.astype(np.int32), step.astype(np.int32), (int(has.sum()), int(step.max()), int(spread.max()))


def classify(counts, elev, step, min_occ=1, min_free=1, occ_ratio=0.0, flags=0, smax=0, **_):
    """int8 [ny, nx]: vg_occupancy's rule on the counts, then flags bit 1's step rule."""
    g = oc.classify(counts, min_occ, min_free, occ_ratio)
    if flags & 2:
        g = np.where((np.asarray(elev) != NONE) & (np.asarray(step, dtype=np.int64) > smax), 100, g).astype(np.int8)
    return g


def _ordered(o, d, ta, tb, ok, x0, y0, res, nx, ny):
    """The pieces of the segments (ta, tb) of the rays `ok` in the order of the walk: (piece [n, K] bool: positive
    length and inside the grid, mid [n, K], ix, iy [n, K] (0 where not a piece))."""
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = (x0 + res * np.arange(nx + 1)[None, :] - o[:, :1]) / d[:, :1]
        ty = (y0 + res * np.arange(ny + 1)[None, :] - o[:, 1:2]) / d[:, 1:2]
    T = np.concatenate([tx, ty], axis=1)
    T[~np.isfinite(T)] = np.inf
    a, b = ta[:, None], tb[:, None]
    S = np.sort(np.concatenate([np.where((T > a) & (T < b), T, np.inf), a, b], axis=1), axis=1)
    lo, hi = S[:, :-1], S[:, 1:]
    live = np.isfinite(hi) & np.isfinite(lo) & ok[:, None]
    with np.errstate(invalid="ignore"):
        piece = live & (hi > lo)
    mid = np.where(piece, 0.5 * (lo + hi), 0.0)
    ix = np.floor((o[:, :1] + mid * d[:, :1] - x0) / res).astype(np.int64)
    iy = np.floor((o[:, 1:2] + mid * d[:, 1:2] - y0) / res).astype(np.int64)
    piece &= (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
    return piece, mid, np.where(piece, ix, 0), np.where(piece, iy, 0)


def terrain(origins, dirs, r, nz, prm, elev=None, ended=None, silent=None, near=None, chunk=1024):
    """origins (n, 3) or (3,), dirs (n, 3); r (n,): the hit's range, inf where the ray has none; nz (n,): the hit
    plane's normal[2]. prm: defaults(...). elev: the elevation pass 2 reads (None: the one of this function's own
    ground planes). ended / silent / near: as occ_ref.marks. Returns a dict: planes (g_n, g_sum, g_min, g_max),
    elev, step, stats (cells_ground, max_step, max_spread), counts int32 [2, ny, nx], uncertain (n,), ground (n,):
    the ray had a ground hit, in_band (n,), carried (n,): the hit was judged with a reference carried from
    another cell, hit_cell (n, 2) ix, iy (outside the grid possible), out_of_range (n,)."""
    P = prm
    x0, y0, res, nx, ny, z_res = P["x0"], P["y0"], P["res"], P["nx"], P["ny"], P["z_res"]
    d = oc._unit(dirs)
    n = d.shape[0]
    o = np.broadcast_to(np.asarray(origins, dtype=np.float64).reshape(-1, 3), d.shape)
    r = np.asarray(r, dtype=np.float64).reshape(n)
    nz = np.asarray(nz, dtype=np.float64).reshape(n)
    ended = np.zeros(n, bool) if ended is None else np.asarray(ended, bool)
    silent = np.zeros(n, bool) if silent is None else np.asarray(silent, bool)
    hit = np.isfinite(r)
    valid = ~ended & (hit | (P["free_on_miss"] > 0.0))
    rh = np.where(hit, r, 0.0)
    dz = d[:, 2]
    hp = o + rh[:, None] * d
    hx = np.floor((hp[:, 0] - x0) / res).astype(np.int64)
    hy = np.floor((hp[:, 1] - y0) / res).astype(np.int64)
    h_in = hit & (hx >= 0) & (hx < nx) & (hy >= 0) & (hy < ny)
    qh = q(hp[:, 2], z_res)
    inr = np.abs(qh) < LIMIT
    # occ_ref's own flags, with a band that cuts nothing
    _, unc, _ = oc.marks(o, d, r, x0, y0, res, nx, ny, z_lo=-1e300, z_hi=1e300, free_on_miss=P["free_on_miss"],
                         t_min=P["t_min"], ended=ended, near=near, chunk=chunk)
    unc = unc.copy()
    mh = hit & ~ended
    unc |= mh & _near_int(hp[:, 2], z_res)
    # pass 1
    rz = rh * dz
    unc |= mh & (np.abs(np.abs(nz) - P["up_min"]) < N_EPS)
    unc |= mh & ((np.abs(rz - P["g_lo"]) < oc.EPS) | (np.abs(rz - P["g_hi"]) < oc.EPS))
    ground = mh & (dz < 0.0) & (np.abs(nz) >= P["up_min"]) & (rz >= P["g_lo"]) & (rz <= P["g_hi"]) & inr & h_in
    g_n = np.zeros((ny, nx), dtype=np.int32)
    g_sum = np.zeros((ny, nx), dtype=np.int64)
    g_min = np.full((ny, nx), 2 ** 31 - 1, dtype=np.int32)
    g_max = np.full((ny, nx), NONE, dtype=np.int32)
    gi = (hy[ground], hx[ground])
    np.add.at(g_n, gi, 1)
    np.add.at(g_sum, gi, qh[ground])
    np.minimum.at(g_min, gi, qh[ground].astype(np.int32))
    np.maximum.at(g_max, gi, qh[ground].astype(np.int32))
    own_elev, step, stats = cells(g_n, g_sum, g_min, g_max, P["min_ground"])
    E = own_elev if elev is None else np.asarray(elev, dtype=np.int32)
    E = E.astype(np.int64)
    # pass 2
    counts = np.zeros((2, ny, nx), dtype=np.int32)
    in_band = np.zeros(n, bool)
    carried = np.zeros(n, bool)
    ref0 = q(o[:, 2] - P["sensor_height"], z_res)
    unc |= valid & _near_int(o[:, 2] - P["sensor_height"], z_res)
    r_end = np.where(hit, r, P["free_on_miss"])
    ta_all = np.full(n, max(P["t_min"], 0.0))
    for c0 in range(0, n, chunk):
        s = slice(c0, min(c0 + chunk, n))
        ok = valid[s] & (ta_all[s] < r_end[s])
        ta, tb = np.where(ok, ta_all[s], 0.0), np.where(ok, r_end[s], 1.0)
        piece, mid, ix, iy = _ordered(o[s], d[s], ta, tb, ok, x0, y0, res, nx, ny)
        K = piece.shape[1]
        e = np.where(piece, E[iy, ix], NONE)
        idx = np.maximum.accumulate(np.where(e != NONE, np.arange(K)[None, :], -1), axis=1)
        rows = np.arange(piece.shape[0])[:, None]
        ref = np.where(idx >= 0, e[rows, np.maximum(idx, 0)], ref0[s][:, None])
        zm = o[s][:, 2:3] + mid * dz[s][:, None]
        qm = q(zm, z_res)
        a = qm - ref
        free = piece & (np.abs(qm) < LIMIT) & (a >= P["clo"]) & (a <= P["chi"])
        unc[s] |= (piece & _near_int(zm, z_res)).any(axis=1)
        # the hit
        ref_end = ref[:, -1]
        he = np.where(h_in[s], E[np.where(h_in[s], hy[s], 0), np.where(h_in[s], hx[s], 0)], NONE)
        href = np.where(he != NONE, he, ref_end)
        ah = qh[s] - href
        ib = hit[s] & valid[s] & inr[s] & (ah >= P["clo"]) & (ah <= P["chi"])
        in_band[s] = ib
        carried[s] = hit[s] & valid[s] & h_in[s] & (he == NONE) & (idx[:, -1] >= 0)
        put = ib & h_in[s]
        np.add.at(counts[1], (hy[s][put], hx[s][put]), 1)
        free &= ~silent[s][:, None]
        own = free & put[:, None] & (ix == hx[s][:, None]) & (iy == hy[s][:, None])
        free &= ~own
        np.add.at(counts[0], (iy[free], ix[free]), 1)
    return dict(planes=(g_n, g_sum, g_min, g_max), elev=own_elev, step=step, stats=stats, counts=counts,
                uncertain=unc, ground=ground, in_band=in_band, carried=carried, hit_cell=np.stack([hx, hy], axis=1),
                out_of_range=mh & ~inr)


def hit_reach(hit_cell, which, nx, ny):
    """[ny, nx] bool: the cells within one cell of the hit cells of the rays `which`."""
    m = np.zeros((ny + 4, nx + 4), bool)
    c = np.asarray(hit_cell)[np.asarray(which, bool)]
    c = c[(c[:, 0] >= -1) & (c[:, 0] <= nx) & (c[:, 1] >= -1) & (c[:, 1] <= ny)]
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            m[c[:, 1] + 2 + a, c[:, 0] + 2 + b] = True
    return m[2:-2, 2:-2]
