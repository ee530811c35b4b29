"""Numpy restatement of the clearance field's definition (vina_gpu.h "Clearance
field and costmap") by brute force: for every cell, all obstacle coordinates and
the lexicographic argmin of (d2, linear index); the cost in double with np.exp.

The device looks the cost up in a table its host filled with libm's exp, which
may differ from numpy's in the last ulp. boundary_free() asserts that no value a
test can meet sits where one ulp could change the byte: no 252 exp(..) within
1e-9 of an integer, no d within 1e-12 of a radius. With that, exact equality of
`cost` is a fair demand."""
import numpy as np

NONE = np.iinfo(np.int32).max            # VG_CLR_NONE
MAX_SIDE = 32768                         # VG_CLR_MAX_SIDE
UNKNOWN, FREE, OCCUPIED = -1, 0, 100     # VG_OCC_*
COST_FREE, COST_INSCRIBED, COST_LETHAL, COST_NO_INFO = 0, 253, 254, 255

# the parameter sets the GPU tests use (tests/test_clearance_gpu.py); test_clr_ref.py holds boundary_free for
# each over every dist2 its table can hold
PARAMS = {
    "nav": dict(res=0.25, inscribed_radius=0.33, inflation_radius=1.9, cost_scaling=3.0),
    "fine": dict(res=0.05, inscribed_radius=0.31, inflation_radius=2.03, cost_scaling=2.5),
    "replay": dict(res=0.2, inscribed_radius=0.33, inflation_radius=1.9, cost_scaling=3.0),
    "none": dict(res=0.25, inscribed_radius=0.0, inflation_radius=0.0, cost_scaling=0.0),
}


def random_grid(nx, ny, seed, p_occ=0.03, p_unknown=0.20, n_other=5):
    """int8 [ny, nx]: about p_occ occupied, p_unknown unknown, the byte value 50 (free) in n_other cells."""
    rng = np.random.default_rng(seed)
    u = rng.random((ny, nx))
    g = np.zeros((ny, nx), dtype=np.int8)
    g[u < p_occ] = OCCUPIED
    g[(u >= p_occ) & (u < p_occ + p_unknown)] = UNKNOWN
    g.ravel()[rng.choice(nx * ny, size=min(n_other, nx * ny), replace=False)] = 50
    return g


def obstacles(grid, flags=0):
    """The obstacle set O as a mask [ny, nx]."""
    g = np.asarray(grid, dtype=np.int8)
    return (g == OCCUPIED) | ((g == UNKNOWN) if flags & 1 else np.zeros(g.shape, dtype=bool))


def transform(grid, flags=0, chunk=1 << 22):
    """(dist2 int32 [ny, nx], nearest int32 [ny, nx]) by brute force."""
    g = np.asarray(grid, dtype=np.int8)
    ny, nx = g.shape
    oi = np.flatnonzero(obstacles(g, flags).ravel())          # ascending: argmin's first hit is the smallest index
    dist2 = np.full(nx * ny, NONE, dtype=np.int32)
    nearest = np.full(nx * ny, -1, dtype=np.int32)
    if oi.size:
        ox, oy = (oi % nx).astype(np.int64), (oi // nx).astype(np.int64)
        step = max(1, chunk // oi.size)
        for c0 in range(0, nx * ny, step):
            c = np.arange(c0, min(c0 + step, nx * ny), dtype=np.int64)
            d2 = ((c % nx)[:, None] - ox[None, :]) ** 2 + ((c // nx)[:, None] - oy[None, :]) ** 2
            j = np.argmin(d2, axis=1)
            dist2[c] = d2[np.arange(c.size), j]
            nearest[c] = oi[j]
    return dist2.reshape(ny, nx), nearest.reshape(ny, nx)


def cost_of(dist2, res, inscribed_radius=0.0, inflation_radius=0.0, cost_scaling=0.0):
    """The cost of a distance alone (before the unknown cells' rule), uint8, same shape as dist2."""
    d2 = np.asarray(dist2, dtype=np.int64)
    d = res * np.sqrt(d2.astype(np.float64))
    skirt = (252.0 * np.exp(-cost_scaling * (d - inscribed_radius))).astype(np.uint8)
    c = np.where(d <= inflation_radius, skirt, COST_FREE)
    c = np.where(d <= inscribed_radius, COST_INSCRIBED, c)
    c = np.where(d2 == 0, COST_LETHAL, c)
    return np.where(d2 == NONE, COST_FREE, c).astype(np.uint8)


def cost(grid, dist2, flags=0, **params):
    """cost uint8 [ny, nx]: cost_of, and 255 on an unknown cell that is no obstacle unless that is >= 253."""
    g = np.asarray(grid, dtype=np.int8)
    c = cost_of(dist2, **params)
    no_info = (g == UNKNOWN) & (c < COST_INSCRIBED)
    return np.where(no_info, COST_NO_INFO, c).astype(np.uint8)


def clearance(grid, flags=0, **params):
    """{dist2, nearest, cost} of the grid."""
    dist2, nearest = transform(grid, flags)
    return dict(dist2=dist2, nearest=nearest, cost=cost(grid, dist2, flags, **params))


def summary(grid, flags, dist2, cost):
    """vg_clr_summary as a dict, counted from the arrays."""
    g = np.asarray(grid, dtype=np.int8)
    n_obst = int(obstacles(g, flags).sum())
    return dict(n_obstacles=n_obst, n_unknown=int((g == UNKNOWN).sum()),
                cells_lethal=int((cost == COST_LETHAL).sum()), cells_inscribed=int((cost == COST_INSCRIBED).sum()),
                cells_inflated=int(((cost > COST_FREE) & (cost < COST_INSCRIBED)).sum()),
                cells_free=int((cost == COST_FREE).sum()), cells_no_info=int((cost == COST_NO_INFO).sum()),
                max_dist2=int(dist2.max()) if n_obst else 0)


def boundary_free(dist2_values, params):
    """Asserts that none of dist2_values (VG_CLR_NONE and 0 aside) puts d within 1e-12 of a radius or 252
    exp(..) within 1e-9 of an integer under params; returns the number of values checked."""
    v = np.unique(np.asarray(dist2_values, dtype=np.int64))
    v = v[(v > 0) & (v != NONE)]
    res, r_in, r_out, k = (params[f] for f in ("res", "inscribed_radius", "inflation_radius", "cost_scaling"))
    d = res * np.sqrt(v.astype(np.float64))
    assert not (np.abs(d - r_in) <= 1e-12).any(), ("d on the inscribed radius", v[np.abs(d - r_in) <= 1e-12])
    assert not (np.abs(d - r_out) <= 1e-12).any(), ("d on the inflation radius", v[np.abs(d - r_out) <= 1e-12])
    skirt = (d > r_in) & (d <= r_out)
    x = 252.0 * np.exp(-k * (d[skirt] - r_in))
    bad = np.abs(x - np.round(x)) <= 1e-9
    assert not bad.any(), ("252 exp(..) on an integer", v[skirt][bad], x[bad])
    return int(v.size)
