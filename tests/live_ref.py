"""Numpy restatement of the live obstacle layer's definition (vina_gpu.h "Live
obstacle layer"): a beam's cells from the closed form (2 k a + n) div (2 n), the
per-point records in double from given classes, the two stamp planes from
records, the live rule and the compose. All beams advance together, one numpy
step per k. test_live_ref.py pins it without a device by hand-worked cases."""
import numpy as np

UNKNOWN, FREE, OCCUPIED = -1, 0, 100                     # VG_OCC_*
DIFF_UNKNOWN, DIFF_CONSISTENT, DIFF_APPEARED, DIFF_VANISHED = 0, 1, 2, 3
MARKS, CLEARS, IN_BAND, CUT, LEFT_BAND = 1, 2, 4, 8, 16  # VG_LIVE_*
CELL_MAX = 1 << 30
MAX_N = 4097
NEAR = 1e-6     # metres: a coordinate this close to a lattice line, or a dz this close to a band limit, is uncertain
REC = np.dtype([("cls", "<i4"), ("flags", "<i4"), ("ax", "<i4"), ("ay", "<i4"), ("bx", "<i4"), ("by", "<i4"),
                ("mx", "<i4"), ("my", "<i4")])


def defaults(res, z_lo=0.0, z_hi=0.0, r_min=0.0, mark_max=0.0, clear_max=0.0, persist=0, flags=0):
    """vg_live_params' defaults applied, as a dict."""
    if z_lo == 0.0 and z_hi == 0.0:
        z_lo, z_hi = -1.0, 1.0
    mm = mark_max if mark_max > 0.0 else np.inf
    cm = clear_max if clear_max > 0.0 else min(4096.0 * res, mm)
    return dict(z_lo=z_lo, z_hi=z_hi, r_min=max(r_min, 0.0), mark_max=mm, clear_max=cm, persist=max(persist, 0),
                flags=flags)


def ray_cells(a, b, with_end=False):
    """The beam's cells c_0 .. c_{n-1} from cell a towards cell b ((n, 2) int64); with_end: c_n = b too."""
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    dx, dy = abs(bx - ax), abs(by - ay)
    n = max(dx, dy)
    sx, sy = (bx > ax) - (bx < ax), (by > ay) - (by < ay)
    ks = range(n + 1 if with_end else n)
    if n == 0:
        return np.array([[ax, ay]] if with_end else [], dtype=np.int64).reshape(-1, 2)
    return np.array([[ax + sx * ((2 * k * dx + n) // (2 * n)), ay + sy * ((2 * k * dy + n) // (2 * n))] for k in ks],
                    dtype=np.int64)


def cell(v, g0, res):
    """floor((v - g0) / res) held to +-2^30, int64."""
    return np.clip(np.floor((np.asarray(v, dtype=np.float64) - g0) / res), -CELL_MAX, CELL_MAX).astype(np.int64)


def points(xyz, pose, ext_R, ext_t, cls, x0, y0, res, **prm):
    """The records (REC [n]) of LiDAR-frame points at pose (12,) from their classes, in double, and the uncertain
    set (bool [n]): a coordinate of o, e or w within NEAR of a lattice line, or dz within NEAR of a band limit."""
    q = defaults(res, **prm)
    R, p = np.asarray(pose[:9], dtype=np.float64).reshape(3, 3), np.asarray(pose[9:12], dtype=np.float64)
    o = R @ ext_t + p
    w = (np.asarray(xyz, dtype=np.float64) @ ext_R.T + ext_t) @ R.T + p
    dv = w - o
    r = np.sqrt((dv * dv).sum(axis=1))
    n = w.shape[0]
    rec = np.zeros(n, dtype=REC)
    rec["cls"] = cls
    fin = np.isfinite(w).all(axis=1) & np.isfinite(o).all()
    dz = dv[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        band = fin & (q["z_lo"] <= dz) & (dz <= q["z_hi"])
        marks_cls = (rec["cls"] == DIFF_APPEARED) | ((q["flags"] & 1) != 0) & (rec["cls"] == DIFF_UNKNOWN)
        marks = band & marks_cls & (q["r_min"] <= r) & (r <= q["mark_max"])
        beam = fin & (r > 0.0)
        t_b = r.copy()
        cut = beam & (q["clear_max"] < t_b)
        t_b[cut] = q["clear_max"]
        t_z = np.where(dz > 0.0, q["z_hi"], q["z_lo"]) * r / dz
        left = beam & (dz != 0.0) & (t_z < t_b)
        t_b[left] = t_z[left]
        cut &= ~left
        f = t_b / r
        e = o[None, :2] + f[:, None] * (w[:, :2] - o[None, :2])
    flags = band * IN_BAND + marks * MARKS + beam * CLEARS + cut * CUT + left * LEFT_BAND
    rec["flags"] = flags
    wf = np.where(fin[:, None], w[:, :2], 0.0)
    rec["mx"] = np.where(fin, cell(wf[:, 0], x0, res), 0)
    rec["my"] = np.where(fin, cell(wf[:, 1], y0, res), 0)
    ef = np.where(beam[:, None], e, 0.0)
    rec["ax"] = np.where(beam, cell(o[0], x0, res), 0)
    rec["ay"] = np.where(beam, cell(o[1], y0, res), 0)
    rec["bx"] = np.where(beam, cell(ef[:, 0], x0, res), 0)
    rec["by"] = np.where(beam, cell(ef[:, 1], y0, res), 0)

    def near_line(v, g0):
        u = (v - g0) / res
        return np.abs(u - np.round(u)) * res <= NEAR

    unc = fin & (near_line(wf[:, 0], x0) | near_line(wf[:, 1], y0))
    unc |= beam & (near_line(o[0], x0) | near_line(o[1], y0) | near_line(ef[:, 0], x0) | near_line(ef[:, 1], y0))
    unc |= fin & ((np.abs(np.where(fin, dz, 0.0) - q["z_lo"]) <= NEAR) | (np.abs(np.where(fin, dz, 0.0) - q["z_hi"]) <= NEAR))
    return rec, unc


def planes(recs, stamp, nx, ny, hit=None, clear=None):
    """(hit, clear) int32 [ny, nx] after the records' marks and beams at `stamp`, from the given planes or zeros.
    Also returns the counts (obstacle points, marks dropped, beams)."""
    hit = np.zeros((ny, nx), dtype=np.int32) if hit is None else np.array(hit, dtype=np.int32)
    clear = np.zeros((ny, nx), dtype=np.int32) if clear is None else np.array(clear, dtype=np.int32)
    r = np.asarray(recs, dtype=REC)
    m = (r["flags"] & MARKS) != 0
    mx, my = r["mx"][m].astype(np.int64), r["my"][m].astype(np.int64)
    inside = (mx >= 0) & (mx < nx) & (my >= 0) & (my < ny)
    np.maximum.at(hit, (my[inside], mx[inside]), stamp)
    b = (r["flags"] & CLEARS) != 0
    ax, ay = r["ax"][b].astype(np.int64), r["ay"][b].astype(np.int64)
    ddx, ddy = r["bx"][b].astype(np.int64) - ax, r["by"][b].astype(np.int64) - ay
    dx, dy, sx, sy = np.abs(ddx), np.abs(ddy), np.sign(ddx), np.sign(ddy)
    n = np.maximum(dx, dy)
    n = np.where(n <= MAX_N, n, 0)           # (never in a record of vg_live_mark: such a beam clears nothing)
    n1 = np.maximum(n, 1)
    for k in range(int(n.max()) if n.size else 0):
        act = k < n
        cx = ax + sx * ((2 * k * dx + n) // (2 * n1))
        cy = ay + sy * ((2 * k * dy + n) // (2 * n1))
        act &= (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
        np.maximum.at(clear, (cy[act], cx[act]), stamp)
    return hit, clear, (int(m.sum()), int((~inside).sum()), int(b.sum()))


def live(hit, clear, now, persist=0):
    """The live cells (bool) at `now`."""
    h, c = np.asarray(hit, dtype=np.int64), np.asarray(clear, dtype=np.int64)
    return (h > 0) & (h >= c) & ((persist == 0) | (now - h < persist))


def compose(base, hit, clear, now, persist=0, flags=0):
    """The composed grid (int8) of vg_live_compose."""
    h, c = np.asarray(hit, dtype=np.int64), np.asarray(clear, dtype=np.int64)
    lv = live(h, c, now, persist)
    out = np.array(base, dtype=np.int8)
    if flags & 1:
        freed = ~lv & (out == UNKNOWN) & (c > 0) & (c > h) & ((persist == 0) | (now - c < persist))
        out[freed] = FREE
    out[lv] = OCCUPIED
    return out
