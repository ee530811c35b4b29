"""A third arithmetic for tests/imu_ref.py: fp64 values that carry a running
bound of their rounding error (Higham, Accuracy and Stability of Numerical
Algorithms, 3.3: every operation adds u |result| to what its operands'
errors propagate to first order; a product of matrices adds n u |A| |B|).
imu_ref.give_evaluate(..., B=ERR) then returns, beside gg = joc^T C r and
r^T C r, what fp64 evaluation of the reference's formulas from the exact
inputs can be off by: the derived bound of tests/test_imu_gpu.py for those
sums. Assumptions, stated: u = 2^-53; sqrt and the four operations rounded
correctly; sin, cos, tan, acos, atan2 within 4 ulp (the device library's
double-precision functions claim 2 or better); derivatives taken at the
computed value (the second-order terms this drops are u times the bound; the
cross terms e_A e_B of products are kept); no
rounding error moves a value across one of the formulas' branch thresholds
(the cases stand 1 % or more away from them)."""
import numpy as np

import f64_ref

U = 2.0 ** -53
FN_ULPS = 4


class E:
    """value v and error bound e (arrays of one shape; scalars are 0-d)."""

    def __init__(self, v, e=None):
        self.v = np.array(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.array(np.broadcast_to(e, self.v.shape), dtype=np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    @property
    def T(self):
        return E(self.v.T, self.e.T)

    def __getitem__(self, k):
        return E(self.v[k], self.e[k])

    def __setitem__(self, k, x):
        x = E.of(x)
        self.v[k], self.e[k] = x.v, x.e

    def __neg__(self):
        return E(-self.v, self.e)

    def __add__(self, o):
        o = E.of(o)
        v = self.v + o.v
        return E(v, self.e + o.e + U * np.abs(v))

    def __sub__(self, o):
        return self + (-E.of(o))

    def __mul__(self, o):  # elementwise / by a scalar
        o = E.of(o)
        v = self.v * o.v
        return E(v, np.abs(self.v) * o.e + self.e * np.abs(o.v) + self.e * o.e + U * np.abs(v))

    __rmul__ = __mul__
    __radd__ = __add__

    def __truediv__(self, o):
        o = E.of(o)
        v = self.v / o.v
        return E(v, self.e / np.abs(o.v) + np.abs(v) * o.e / np.abs(o.v) + U * np.abs(v))


def fn(x, f, df):
    v = f(x.v)
    return E(v, np.abs(df(x.v)) * x.e + FN_ULPS * U * np.abs(v))


def mm(*ms):
    out = ms[0]
    for b in ms[1:]:
        a, n = out, out.v.shape[1]
        out = E(a.v @ b.v, np.abs(a.v) @ b.e + a.e @ np.abs(b.v) + a.e @ b.e + n * U * (np.abs(a.v) @ np.abs(b.v)))
    return out


def norm(v):
    n = np.sqrt((v.v ** 2).sum())
    return E(n, (np.abs(v.v) * v.e).sum() / n + 3 * U * n) if n > 0 else E(0.0, np.sqrt((v.e ** 2).sum()))


def hat(v):
    z = E(0.0)
    a = [v[i, 0] for i in range(3)]
    rows = [[z, -a[2], a[1]], [a[2], z, -a[0]], [-a[1], a[0], z]]
    return E([[c.v for c in r] for r in rows], [[c.e for c in r] for r in rows])


def eye(n):
    return E(np.eye(n))


def _rodrigues(axis, s, c1):
    """I + s K + c1 K K (math.hpp's Exp), K = hat(axis)."""
    K = hat(axis)
    return eye(3) + K * s + mm(K, K) * c1


def Exp(v):
    n = norm(v)
    if n.v < 1e-9:
        return eye(3)
    return _rodrigues(v / n, fn(n, np.sin, np.cos), E(1.0) - fn(n, np.cos, np.sin))


def Log(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    K = E(np.zeros((3, 1)))
    for i, (a, b) in enumerate((((2, 1), (1, 2)), ((0, 2), (2, 0)), ((1, 0), (0, 1)))):
        K[i, 0] = R[a] - R[b]
    if tr.v > 3.0 - 1e-6:
        return K * 0.5
    x = (tr - 1.0) * 0.5
    th = fn(x, np.arccos, lambda t: 1.0 / np.sqrt(1.0 - t * t))
    if abs(th.v) < 0.001:
        return K * 0.5
    return K * (th * 0.5 / fn(th, np.sin, np.cos))


def jr(v):
    a = norm(v)
    if a.v < 1e-9:
        return eye(3)
    u = v / a
    ra = fn(a, np.sin, np.cos) / a
    return eye(3) * ra + mm(u, u.T) * (E(1.0) - ra) - hat(u) * ((E(1.0) - fn(a, np.cos, np.sin)) / a)


def jr_inv(R):
    q = [E(0.0)] * 4  # Eigen::AngleAxisd(Matrix3d), through the quaternion (f64_ref.jr_inv's branches)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    sq = lambda x: fn(x, np.sqrt, lambda y: 0.5 / np.sqrt(y))
    if t.v > 0:
        t = sq(t + 1.0)
        q[3] = t * 0.5
        t = E(0.5) / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R.v[1, 1] > R.v[0, 0]:
            i = 1
        if R.v[2, 2] > R.v[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = sq(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = t * 0.5
        t = E(0.5) / t
        q[3], q[j], q[k] = (R[k, j] - R[j, k]) * t, (R[j, i] + R[i, j]) * t, (R[k, i] + R[i, k]) * t
    qv = E([[c.v] for c in q[:3]], [[c.e] for c in q[:3]])
    n = norm(qv)
    if n.v == 0.0:
        return eye(3)
    w, d = abs(q[3].v), n.v ** 2 + q[3].v ** 2
    ang = E(2.0 * np.arctan2(n.v, w), 2.0 * (w * n.e + n.v * q[3].e) / d + 2 * FN_ULPS * U * np.arctan2(n.v, w))
    ax = qv / (n if q[3].v >= 0 else -n)
    if ang.v < 1e-9:
        return eye(3)
    h = ang * 0.5
    ctt = h / fn(h, np.tan, lambda y: 1.0 / np.cos(y) ** 2)
    return eye(3) * ctt + mm(ax, ax.T) * (E(1.0) - ctt) + hat(ax) * h


class ERR:
    """imu_ref's backend: fp64 with running error bounds."""
    name = "err"
    num = staticmethod(lambda x: x if isinstance(x, E) else E(float(x)))

    @staticmethod
    def mat(a):
        a = np.array(a, dtype=np.float64)
        return E(a[:, None] if a.ndim == 1 else a)

    zeros = staticmethod(lambda r, c: E(np.zeros((r, c))))
    eye = staticmethod(eye)
    mm = staticmethod(mm)
    hat = staticmethod(hat)
    Exp = staticmethod(Exp)
    Log = staticmethod(Log)
    jr = staticmethod(jr)
    jr_inv = staticmethod(jr_inv)


def self_check():
    """The values this arithmetic carries are f64_ref's (same formulas, same branches)."""
    rng = np.random.default_rng(0)
    for a in (0.0, 1e-10, 5e-4, 2e-3, 0.5, 3.0):
        w = rng.normal(size=3)
        w *= a / np.linalg.norm(w)
        R = f64_ref.Exp(w)
        assert np.allclose(Exp(ERR.mat(w)).v, R, rtol=0, atol=1e-15)
        assert np.allclose(Log(E(R)).v[:, 0], f64_ref.Log(R), rtol=0, atol=1e-14)
        assert np.allclose(jr(ERR.mat(w)).v, f64_ref.jr(w), rtol=0, atol=1e-15)
        assert np.allclose(jr_inv(E(R)).v, f64_ref.jr_inv(R), rtol=0, atol=1e-12)
