"""numpy restatement of the place index (vina_gpu.h "Place index"; csrc/vg_place.h,
places.hip): the direction table, a place's descriptor from ranges, the scan's
binning and the integer match. Everything after the geometry is integer
arithmetic, so the device's descriptors and scores are compared for equality.

Layout: a descriptor is (E, A) uint16, range in 1/512 m, 0 = none. Azimuth bin
a covers [a, a + 1) 2 pi / A from the frame's x axis about `up`; elevation bin e
covers el_min + [e, e + 1) (el_max - el_min) / E. The frame: up = -g / |g|,
x = world x made perpendicular to up, y = up x x."""
import math

import numpy as np

Q = 512            # quantisation steps per metre
INT32_MAX = 2 ** 31 - 1
DEFAULTS = dict(n_az=120, n_el=12, el_min=math.radians(-30.0), el_max=math.radians(30.0), t_max=60.0, clip=2.0,
                min_bins=0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    if p["min_bins"] <= 0:
        p["min_bins"] = max(1, p["n_az"] * p["n_el"] // 8)
    return p


def frame(g=(0.0, 0.0, -9.8)):
    """(3, 3) rows ex, ey, up."""
    g = np.asarray(g, dtype=np.float64)
    gn = math.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
    up = -g / gn if gn > 0 else np.array([0.0, 0.0, 1.0])
    ref = np.array([1.0, 0.0, 0.0]) if abs(up[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    c = ref[0] * up[0] + ref[1] * up[1] + ref[2] * up[2]
    ex = ref - c * up
    ex = ex / math.sqrt(ex[0] * ex[0] + ex[1] * ex[1] + ex[2] * ex[2])
    ey = np.array([up[1] * ex[2] - up[2] * ex[1], up[2] * ex[0] - up[0] * ex[2], up[0] * ex[1] - up[1] * ex[0]])
    return np.stack([ex, ey, up])


def dirs(p):
    """(E * A, 3) bin-centre directions in the descriptor's own frame (x, y, up), bin e * A + a."""
    A, E = p["n_az"], p["n_el"]
    out = np.zeros((E * A, 3))
    w = 2.0 * math.pi / A
    h = (p["el_max"] - p["el_min"]) / E
    for e in range(E):
        el = p["el_min"] + (e + 0.5) * h
        for a in range(A):
            az = (a + 0.5) * w
            out[e * A + a] = (math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el))
    return out


def quantise(ranges):
    """Ranges in metres (inf / nan / <= 0: none) -> uint16 steps, clipped."""
    r = np.asarray(ranges, dtype=np.float64)
    ok = np.isfinite(r) & (r > 0)
    q = np.zeros(r.shape, dtype=np.int64)
    q[ok] = np.minimum(np.rint(Q * r[ok]).astype(np.int64), 65535)
    return q.astype(np.uint16)


def mat3(a, b):
    """a @ b for 3 x 3 in the library's order of operations (vg_la.h mul)."""
    o = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            s = a[i, 0] * b[0, j]
            for k in range(1, 3):
                s += a[i, k] * b[k, j]
            o[i, j] = s
    return o


def scan_bins(xyz, R_level, ext_R, p, g=(0.0, 0.0, -9.8)):
    """Per point: (bin index or -1, q, az, el, r). xyz float32 (n, 3) in the LiDAR frame."""
    A, E = p["n_az"], p["n_el"]
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    M = mat3(np.asarray(R_level, dtype=np.float64).reshape(3, 3), np.asarray(ext_R, dtype=np.float64).reshape(3, 3))
    F = frame(g)
    v = [M[i, 0] * x[:, 0] + M[i, 1] * x[:, 1] + M[i, 2] * x[:, 2] for i in range(3)]
    r = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    cx = F[0, 0] * v[0] + F[0, 1] * v[1] + F[0, 2] * v[2]
    cy = F[1, 0] * v[0] + F[1, 1] * v[1] + F[1, 2] * v[2]
    cz = F[2, 0] * v[0] + F[2, 1] * v[1] + F[2, 2] * v[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        az = np.arctan2(cy, cx)
        az = np.where(az < 0, az + 2.0 * math.pi, az)
        el = np.arcsin(cz / r)
        w = 2.0 * math.pi / A
        h = (p["el_max"] - p["el_min"]) / E
        a = np.minimum(np.floor(az / w), A - 1)
        e = np.floor((el - p["el_min"]) / h)
    ok = (r > 0) & (r <= p["t_max"]) & (e >= 0) & (e < E) & np.isfinite(az) & np.isfinite(el)
    b = np.where(ok, e * A + a, -1).astype(np.int64)
    q = np.minimum(np.rint(Q * np.where(ok, r, 0.0)), 65535).astype(np.int64)
    return b, q, az, el, r


def scan_descriptor(xyz, R_level, ext_R, p, g=(0.0, 0.0, -9.8), skip=None):
    """(desc (E, A) uint16, n (E, A) int32). skip: points left out (bool mask)."""
    A, E = p["n_az"], p["n_el"]
    b, q, _, _, _ = scan_bins(xyz, R_level, ext_R, p, g)
    keep = b >= 0
    if skip is not None:
        keep &= ~skip
    n = np.bincount(b[keep], minlength=A * E).astype(np.int64)
    s = np.zeros(A * E, dtype=np.int64)
    np.add.at(s, b[keep], q[keep])
    d = np.zeros(A * E, dtype=np.int64)
    nz = n > 0
    d[nz] = np.minimum((s[nz] + n[nz] // 2) // n[nz], 65535)
    return d.astype(np.uint16).reshape(E, A), n.astype(np.int32).reshape(E, A)


def edge_mask(xyz, R_level, ext_R, p, g=(0.0, 0.0, -9.8), eps_ang=1e-9, eps_r=1e-9):
    """Points within eps_ang of a bin edge (azimuth or elevation, the span's ends included) or eps_r of t_max."""
    A, E = p["n_az"], p["n_el"]
    _, _, az, el, r = scan_bins(xyz, R_level, ext_R, p, g)
    w = 2.0 * math.pi / A
    h = (p["el_max"] - p["el_min"]) / E
    fa = az / w
    fe = (el - p["el_min"]) / h
    da = np.abs(fa - np.rint(fa)) * w
    de = np.abs(fe - np.rint(fe)) * h
    inside = (fe > -1) & (fe < E + 1)
    return (da <= eps_ang) | ((de <= eps_ang) & inside) | (np.abs(r - p["t_max"]) <= eps_r) | ~np.isfinite(el)


def match_scores(place_desc, scan_desc, clip_q):
    """scores (M, A) int64: place_desc (M, E, A) uint16, scan_desc (E, A) uint16.
    score(s) = sum over scan-valid bins of min(|place[e][(a + s) % A] - scan[e][a]|, clip_q); an empty place
    bin under a valid scan bin is charged clip_q."""
    P = np.asarray(place_desc, dtype=np.int64)
    S = np.asarray(scan_desc, dtype=np.int64)
    M, E, A = P.shape
    sv = S > 0
    out = np.zeros((M, A), dtype=np.int64)
    for s in range(A):
        Ps = np.roll(P, -s, axis=2)  # Ps[m, e, a] = P[m, e, (a + s) % A]
        c = np.minimum(np.abs(Ps - S[None]), clip_q)
        c = np.where(Ps == 0, clip_q, c)
        out[:, s] = np.where(sv[None], c, 0).sum(axis=(1, 2))
    return out


def best_two(scores_row):
    """((s0, score0), (s1, score1)) of one place's A scores: the best shift (ties to the lower s) and the best
    shift at least A / 4 bins (circularly) away from it; (-1, INT32_MAX) where there is none."""
    A = scores_row.shape[0]
    s0 = int(np.argmin(scores_row))
    d = np.abs(np.arange(A) - s0)
    d = np.minimum(d, A - d)
    far = 4 * d >= A
    if not far.any():
        return (s0, int(scores_row[s0])), (-1, INT32_MAX)
    masked = np.where(far, scores_row, np.iinfo(np.int64).max)
    s1 = int(np.argmin(masked))
    return (s0, int(scores_row[s0])), (s1, int(scores_row[s1]))


def top_k(scores, valid, k):
    """The k smallest (score, place, shift) records over both per-place entries of the valid places."""
    rec = []
    for m in range(scores.shape[0]):
        if not valid[m]:
            continue
        for s, sc in best_two(scores[m]):
            if s >= 0:
                rec.append((sc, m, s))
    rec.sort()
    return rec[:k]


def hit_bins(place_desc):
    return (np.asarray(place_desc).reshape(place_desc.shape[0], -1) > 0).sum(axis=1).astype(np.int32)


def lattice(lo, hi, step, z):
    """(M, 3) positions, x fastest: lo / hi (2,) inclusive bounds."""
    nx = int(math.floor((hi[0] - lo[0]) / step + 1e-9)) + 1
    ny = int(math.floor((hi[1] - lo[1]) / step + 1e-9)) + 1
    out = np.zeros((nx * ny, 3))
    k = 0
    for j in range(ny):
        for i in range(nx):
            out[k] = (lo[0] + i * step, lo[1] + j * step, z)
            k += 1
    return out


def rot_up(yaw, g=(0.0, 0.0, -9.8)):
    """Rotation by yaw about up."""
    u = frame(g)[2]
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + math.sin(yaw) * K + (1 - math.cos(yaw)) * (K @ K)
