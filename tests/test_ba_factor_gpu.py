"""The LM's LiDAR factor passes on given factors: k_ba_resid, then k_ba_hess +
k_ba_hfinal (hess_chunk_eval, factor_frame; ba_factor.hip) through
vgx_ba_factors, which runs them by the body the host-driven LM's passes use.
W = 2, 3, 5, 8, 9, 11 (hess_fs 64, 64, 64, 64, 56, 46 factors per chunk; 1, 2,
2, 3, 4, 5 MFMA tiles; W = 8 the only window whose 6W is a multiple of 16; W =
10 is what every workload runs).

References. A factor set's Hessian, gradient and residual: the sum over the
factors of oracle.kat_lidar_factor (math.fsum per entry); fac_eig / fac_pcr:
oracle.kat_lidar_eig. On each case's small subset (at most 8 factors) the
50-digit tests/factor_ref.py gives the oracle's own fp64 error, and the device
is run on that subset and compared with the 50-digit values directly.

Bounds. Hessian and gradient per 6 x 6 block / 6-slice, relative to the
reference block's largest entry; eigenvalues relative to the factor's largest;
eigenvectors entry-wise after the sign is taken from u . u_ref. The device is
allowed 8 times the oracle's error on the case's subset, with a floor of 1e-13
(_rule). The full-size sets' Hessian and gradient are compared with the oracle
under the same allowance (the factors of a set are one population; the terms of
a block add with the block, so the error relative to the block's largest entry
does not grow with the factor count). Their fac_eig is compared with the
50-digit eigen system of every factor (the merge and eigsy alone, a few ms
each) under the oracle's error on those same factors: an eigenvector's error
goes with 1 / gap of its own factor, which a subset of 4 does not bound (first
run: 1.2e-13 between device and oracle at one of 199 factors, W = 3, where the
subset's oracle error was 4e-15). A block whose reference is exactly zero must be
exactly 0.0 on the device, and each case asserts how many such blocks it has.
Residual sums: |sum - fsum(the device's own lambda_min)| <= n 2^-53 sum|terms|
(a fixed-order sum of n terms). fac_pcr: (12 W + 4) 2^-53 sum|terms| per entry,
the terms being the elementary products of PointCluster::transform and the
merge (each entry sums at most 12 W + 1 of them, each rounded at most 3 times);
against the oracle twice that (both sides round).

Observed on an MI355X (printed by every run as RULE / RESID lines: device
error, oracle error, their ratio), the worst over W of device / oracle, and the
errors there. The allowance is 8 (or the floor):
  a generic      H 1.1 (2.0e-14)  g 3.0 (1.5e-13 / 4.9e-14)  eigenvalues 1.1 (8.5e-14)  eigenvectors 1.9 (4.2e-13)
  d sparse       H 1.6 (2.1e-14)  g 2.0 (7.7e-14)            eigenvalues 1.5 (2.0e-14)  eigenvectors 1.9 (1.1e-13)
  e indexing     H 1.0            g 1.1                      eigenvalues 1.2            eigenvectors 1.9
  f gap 1e3      H 1.0 (1.3e-13)  g 1.5 (2.3e-12)           eigenvalues 1.0            eigenvectors 1.2
  f gap 2        H 1.4 (3.7e-14)  g 2.3 (8.8e-14)            eigenvalues 1.1            eigenvectors 1.2
  f gap 1+1e-3   H 1.2 (2.3e-10)  g 1.4 (2.0e-10)            eigenvalues 1.3 (1.5e-13)  eigenvectors 1.4 (3.5e-11)
  f 500 m        H 1.0 (4.4e-10)  g 1.2 (6.7e-10)            eigenvalues 1.1 (2.2e-12)  eigenvectors 1.0 (1.4e-10)
The 1 + 1e-3 gap and the 500 m clusters cost the device and the oracle alike
(1e-10 instead of 1e-14): the rule needs no widening there. Residual sums: at
most 0.44 of the bound. Every bit-identity assertion (G, nrb, the ring, node
ids, repeated calls) held.

Deliberately wrong edits of ba_factor.hip, each run against this file: g1 / g2
row strides swapped — a, d, e, f fail at every W; `i` for `mpring[i]` and
fac_eig indexed by node — e fails at every W (the ring and the node-id runs).
Dropping the `row / 6 != colx / 6` filter changes no output: the diagonal
blocks the MFMA tiles would then store are overwritten by the register-summed
ones behind the workgroup barrier that separates the two groups of stores, so
the filter saves stores and no test can tell.
"""
import math

import numpy as np
import pytest

import factor_ref as fr
import lm_ref
import oracle
import synth
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
FLOOR = 1e-13
WINS = [2, 3, 5, 8, 9, 11]
RESID_BLOCKS = 512   # vg_ba.h kResidBlocks
HESS_GRID_MAX = 256  # vg_ba.h kHessGridMax


def hess_fs(W):
    """vg_ba.h hess_fs: the Hessian pass's factors per chunk."""
    two = 2 * (256 // W)
    return two if two <= 64 and two <= 512 // W else min(512 // W, 64)


def test_chunk_formulas():
    assert [hess_fs(W) for W in (2, 3, 5, 8, 9, 10, 11)] == [64, 64, 64, 64, 56, 50, 46]
    assert [(6 * W + 15) // 16 for W in (2, 3, 5, 8, 9, 10, 11)] == [1, 2, 2, 3, 4, 4, 5]


_ctxs = {}
_cache = {}


@pytest.fixture(scope="module")
def ctx_for():
    def get(W):
        if W not in _ctxs:
            p = vgconfig.load("mid360")
            p["LocalBA"]["win_size"] = W
            _ctxs[W] = vgpu.Context(vgconfig.to_c(p), max_points=20_000, max_nodes=100_000, max_fix_points=200_000,
                                    hash_log2=16)
        return _ctxs[W]
    yield get
    for c in _ctxs.values():
        c.close()
    _ctxs.clear()
    _cache.clear()


# ---- running a factor set ----------------------------------------------------------------------------------

class Set:
    """Factors (clus (W, 13) by frame, fix (13,)) at shared window poses (W, 12)."""

    def __init__(self, W, poses, factors, seed):
        self.W, self.poses, self.factors = W, poses, factors
        self.xs = fr.states(poses, np.random.default_rng(seed))
        self._orc = None

    def sub(self, idx):
        s = Set(self.W, self.poses, [self.factors[i] for i in idx], 0)
        s.xs = self.xs
        if self._orc is not None:
            s._orc = [self._orc[i] for i in idx]
        return s

    def orc(self):
        """Per factor: (lambda_min, J, H, eig 12, pcr 13) from the oracle, computed once."""
        if self._orc is None:
            self._orc = [oracle.kat_lidar_factor(c, f, self.poses) + oracle.kat_lidar_eig(c, f, self.poses)
                         for c, f in self.factors]
        return self._orc


def _fsum_cols(rows):
    a = np.asarray(rows, dtype=np.float64).reshape(len(rows), -1)
    return np.array([math.fsum(a[:, k]) for k in range(a.shape[1])])


def _orc_out(s, nf=None):
    """The oracle's result for the first nf factors, in the device result's form."""
    o = s.orc()[: len(s.factors) if nf is None else nf]
    L = 6 * s.W
    iu = np.tril_indices(L)
    H = np.zeros((L, L))
    H[iu] = _fsum_cols([x[2][iu] for x in o])
    H = H + np.tril(H, -1).T
    return {"H": H, "g": _fsum_cols([x[1] for x in o]), "eig": np.array([x[3] for x in o]),
            "pcr": fr.to_dev(np.array([x[4] for x in o]))}


def _run(ctx, s, nf=None, ring=None, node_ids=None, order=None, G=0, nrb=0, decoys=None):
    """The first nf factors of s on the device. ring: frame -> physical slot; node_ids: each factor's
    node; order: the factor order (indices into the set); decoys: (node ids, (clus, fix)) written to the
    map beside the set's nodes and used by no factor."""
    W = s.W
    n = len(s.factors) if nf is None else nf
    ring = np.arange(W) if ring is None else np.asarray(ring)
    node_ids = np.arange(n) if node_ids is None else np.asarray(node_ids)[:n]
    order = np.arange(n) if order is None else np.asarray(order)
    clus = np.zeros((n, W, 10))
    fix = np.zeros((n, 10))
    for a in range(n):
        c, f = s.factors[a]
        clus[a, ring] = fr.to_dev(c)  # frame i's cluster lives in slot ring[i]
        fix[a] = fr.to_dev(f)
    nodes = node_ids
    if decoys is not None:
        dn, (dc, df) = decoys
        dclus = np.zeros((len(dn), W, 10))
        dclus[:, ring] = fr.to_dev(dc)
        nodes = np.r_[node_ids, dn]
        clus = np.concatenate([clus, dclus])
        fix = np.concatenate([fix, np.tile(fr.to_dev(df), (len(dn), 1))])
    o = ctx.ba_factors(W, node_ids[order], nodes, clus, fix, s.xs, ring, G, nrb)
    o["H"] = lm_ref.unpack_lower(o["H"], 6 * W)
    return o


# ---- errors and the rule -----------------------------------------------------------------------------------

def _diff(dev, ref):
    """|dev - ref| and |ref| as fp64 arrays of dev's shape; ref fp64, or an mpmath matrix / list."""
    dev = np.asarray(dev, dtype=np.float64)
    if isinstance(ref, np.ndarray):
        return np.abs(dev - ref), np.abs(ref)
    flat = list(ref)
    assert len(flat) == dev.size
    d = np.array([float(abs(fr.mp.mpf(float(x)) - r)) for x, r in zip(dev.ravel(), flat)]).reshape(dev.shape)
    return d, np.array([float(abs(r)) for r in flat]).reshape(dev.shape)


def _block_err(W, dev, ref, zeros):
    """The largest error of a 6 x 6 block of the Hessian (or 6-slice of the gradient) relative to the
    reference block's largest entry. A block whose reference is exactly zero must be exactly 0.0 in
    dev; `zeros` is how many such blocks the case has."""
    d, r = _diff(dev, ref)
    dev = np.asarray(dev)
    worst, nz = 0.0, 0
    cols = range(W) if dev.ndim == 2 and dev.shape[1] > 1 else [None]
    for i in range(W):
        for j in cols:
            sl = (slice(6 * i, 6 * i + 6),) + (() if j is None else (slice(6 * j, 6 * j + 6),))
            if r[sl].max() == 0.0:
                assert np.all(dev[sl] == 0.0), (i, j)
                nz += 1
            else:
                worst = max(worst, float(d[sl].max() / r[sl].max()))
    assert nz == zeros, (nz, zeros)
    return worst


def _eig_err(dev, ref_w, ref_U):
    """(eigenvalue error relative to the largest, eigenvector error after the sign from u . u_ref) over the
    factors; ref_w / ref_U per factor, fp64 arrays or mpmath."""
    ew = eu = 0.0
    for e, w, U in zip(dev, ref_w, ref_U):
        d, r = _diff(e[:3], w if isinstance(w, np.ndarray) else fr.mp.matrix(w))
        ew = max(ew, float(d.max() / r.max()))
        Ud = e[3:].reshape(3, 3)
        Ur = U if isinstance(U, np.ndarray) else np.array([[float(U[a, b]) for b in range(3)] for a in range(3)])
        sg = np.sign(np.sum(Ud * Ur, axis=0))
        assert np.all(sg != 0)
        d, _ = _diff(Ud * sg, U if isinstance(U, np.ndarray) else fr.mp.matrix(U))
        eu = max(eu, float(d.max()))
    return ew, eu


def _errs(W, out, ref, zeros=(0, 0)):
    """out against ref = {"H", "g", "w", "U"} -> the four errors."""
    ew, eu = _eig_err(out["eig"], ref["w"], ref["U"])
    return {"H": _block_err(W, out["H"], ref["H"], zeros[0]),
            "g": _block_err(W, out["g"].reshape(-1, 1), ref["g"], zeros[1]), "w": ew, "U": eu}


def _mp_ref(s):
    H, J, _, per = fr.evaluate_sum(s.factors, s.poses)
    return {"H": H, "g": J, "w": [o["w"] for o in per], "U": [o["U"] for o in per], "pcr": [o["pcr"] for o in per]}


def _rule(tag, dev, orc):
    """Each of the device's errors at most 8 times the oracle's, floor 1e-13."""
    for k in ("H", "g", "w", "U"):
        print("RULE %s %s: device %.2e oracle %.2e ratio %.2f" % (tag, k, dev[k], orc[k], dev[k] / max(orc[k], FLOOR / 8)))
    for k in ("H", "g", "w", "U"):
        assert dev[k] <= max(8 * orc[k], FLOOR), (tag, k, dev[k], orc[k])


def _subset_rule(ctx, tag, s, zeros=(0, 0), **kw):
    """The device on the (small) set s against the 50-digit reference, allowed 8 times the oracle's own
    error on s. Returns (the device result, the oracle's errors)."""
    assert len(s.factors) <= 8
    ref = _mp_ref(s)
    e_orc = _errs(s.W, _orc_out(s), ref, zeros)
    out = _run(ctx, s, **kw)
    order = kw.get("order")  # the per-factor outputs back in the set's order
    _rule(tag, _errs(s.W, out if order is None else {**out, "eig": out["eig"][np.argsort(order)]}, ref, zeros), e_orc)
    _check_pcr(s, out, ref["pcr"], kw.get("order"))
    _check_resid(tag, out)
    return out, e_orc


def _check_resid(tag, out):
    """Both residual sums against the exact sum of the device's own smallest eigenvalues."""
    lam = out["eig"][:, 0] if len(out["eig"]) else np.zeros(0)
    exact, bound = math.fsum(lam), len(lam) * U53 * math.fsum(np.abs(lam))
    for k in ("res", "resid"):
        e = abs(out[k] - exact)
        print("RESID %s %s: |sum - exact| %.2e bound %.2e" % (tag, k, e, bound))
        assert e <= bound, (tag, k, out[k], exact, bound)


def _pcr_terms(s):
    """Per factor: sum |terms| of each fac_pcr entry (10) — the elementary products of transform and the merge."""
    out = []
    for c, f in s.factors:
        P, v = np.abs(f[:9].reshape(3, 3)), np.abs(f[9:12])
        for ci, x in zip(c, s.poses):
            if ci[12] == 0:
                continue
            R, p = np.abs(x[:9].reshape(3, 3)), np.abs(x[9:12])
            Rv = R @ np.abs(ci[9:12])
            P = P + R @ np.abs(ci[:9].reshape(3, 3)) @ R.T + np.outer(Rv, p) + np.outer(p, Rv) + ci[12] * np.outer(p, p)
            v = v + Rv + ci[12] * p
        out.append(np.r_[P[np.triu_indices(3)], v, 0.0])
    return np.array(out)


def _check_pcr(s, out, ref, order=None, factor=1):
    """fac_pcr against the 50-digit merge (ref: (P, v, N) per factor), or against the oracle's (ref: an
    (n, 10) array, factor = 2)."""
    n = len(out["pcr"])
    idx = np.arange(n) if order is None else np.asarray(order)
    bound = factor * (12 * s.W + 4) * U53 * _pcr_terms(s)
    for a in range(n):
        r = ref[idx[a]]
        if not isinstance(r, np.ndarray):
            P, v, N = r
            r = fr.mp.matrix([P[0, 0], P[0, 1], P[0, 2], P[1, 1], P[1, 2], P[2, 2], v[0], v[1], v[2], N])
        d, _ = _diff(out["pcr"][a], r)
        assert d[9] == 0.0 and np.all(d <= bound[idx[a]]), (a, d, bound[idx[a]])


def _same(a, b, keys=("H", "g", "res", "resid", "eig", "pcr")):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys)


# ---- the sets ----------------------------------------------------------------------------------------------

def _generic(W):
    """3 C + 7 plane voxels of random orientation, every frame populated (case a, c)."""
    key = ("generic", W)
    if key not in _cache:
        rng = np.random.default_rng(1000 + W)
        true, poses = fr.window(rng, W)
        n = 3 * hess_fs(W) + 7
        _cache[key] = Set(W, poses, [fr.plane_factor(rng, true) for _ in range(n)], W)
    return _cache[key]


def _generic_err(ctx, W):
    """The oracle's error on the generic set's first 4 factors, with the device held to the rule there."""
    key = ("generic-err", W)
    if key not in _cache:
        _cache[key] = _subset_rule(ctx, "a W %d subset" % W, _generic(W).sub(range(4)))[1]
    return _cache[key]


def _generic_eig(W):
    """Every generic factor's 50-digit eigen system (the merge and mpmath.eigsy alone: a few ms each) and
    the oracle's own error on it, (n, 2): eigenvalues, eigenvectors. An eigenvector's error goes with
    1 / gap of its own factor, so the worst of 3 C + 7 factors is not seen on a subset of 4."""
    key = ("generic-eig", W)
    if key not in _cache:
        s = _generic(W)
        ref = [fr.eigen(fr.merge(c, f, s.poses)) for c, f in s.factors]
        _cache[key] = ref, np.array([_eig_err([o[3]], [w], [U]) for o, (w, U) in zip(s.orc(), ref)])
    return _cache[key]


def _full_rule(ctx, tag, W, out, nf):
    """The device on the generic set's first nf factors (out, in the set's order): Hessian and gradient
    against the oracle's sums, allowed 8 times the oracle's error on the subset; fac_eig against the
    50-digit eigen systems, allowed 8 times the oracle's error on the same nf factors."""
    s = _generic(W)
    ref, eo = _generic_eig(W)
    o = _orc_out(s, nf)
    ew, eu = _eig_err(out["eig"], [r[0] for r in ref[:nf]], [r[1] for r in ref[:nf]])
    dev = {"H": _block_err(W, out["H"], o["H"], 0), "g": _block_err(W, out["g"].reshape(-1, 1), o["g"].reshape(-1, 1), 0),
           "w": ew, "U": eu}
    e_sub = _generic_err(ctx, W)
    _rule(tag, dev, {"H": e_sub["H"], "g": e_sub["g"], "w": float(eo[:nf, 0].max()), "U": float(eo[:nf, 1].max())})
    _check_pcr(s, out, o["pcr"], factor=2)


# ---- a. generic planes at the chunk boundaries ---------------------------------------------------------------

@pytest.mark.parametrize("W", WINS)
def test_generic_planes(oracle_lib, ctx_for, W):
    ctx, s = ctx_for(W), _generic(W)
    C, c = hess_fs(W), 256 // W
    for nf in sorted({1, C - 1, C, C + 1, c - 1, c, c + 1, 3 * C + 7}):
        out = _run(ctx, s, nf)
        _full_rule(ctx, "a W %d nf %d" % (W, nf), W, out, nf)
        _check_resid("a W %d nf %d" % (W, nf), out)
        assert out["eig"].shape == (nf, 12)


# ---- b. no factors -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", WINS)
def test_no_factors(oracle_lib, ctx_for, W):
    ctx, s = ctx_for(W), _generic(W)
    assert _run(ctx, s, hess_fs(W) + 1)["res"] > 0.0  # the partials and sums hold values from a real set
    out = _run(ctx, s, 0)
    assert np.all(out["H"] == 0.0) and np.all(out["g"] == 0.0) and out["res"] == 0.0 and out["resid"] == 0.0
    assert not np.signbit(out["H"]).any() and not np.signbit(out["g"]).any()


# ---- c. the chunk loop ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", WINS)
def test_chunk_loop(oracle_lib, ctx_for, W):
    ctx, s = ctx_for(W), _generic(W)
    base = _run(ctx, s)
    assert _same(base, _run(ctx, s))  # two identical calls
    for G in (1, 2, HESS_GRID_MAX):
        o = _run(ctx, s, G=G)
        assert _same(base, o, ("H", "g", "res", "eig", "pcr")), G  # chunk c -> partial c whatever G
    lam = base["eig"][:, 0]
    bound = len(lam) * U53 * math.fsum(np.abs(lam))
    for nrb in (1, 3, RESID_BLOCKS):
        o = _run(ctx, s, nrb=nrb)
        assert _same(base, o, ("H", "g", "res", "eig", "pcr")), nrb
        _check_resid("c W %d nrb %d" % (W, nrb), o)
        assert abs(o["resid"] - base["resid"]) <= 2 * bound


# ---- d. sparse frames ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", WINS)
def test_sparse_frames(oracle_lib, ctx_for, W):
    ctx = ctx_for(W)
    rng = np.random.default_rng(2000 + W)
    true, poses = fr.window(rng, W)
    # exactly one frame (first, middle, last), with a populated and with an empty fixed cluster; exactly two
    facs, seen = [], np.zeros((W, W), dtype=bool)
    for frames, n_fix in (((0,), 20), ((W // 2,), 0), ((W - 1,), 20), ((0,), 0), ((W - 1,), 0),
                          ((0, W - 1), 0), ((W // 2, W - 1), 20)):
        facs.append(fr.plane_factor(rng, true, fr.sparse_counts(W, frames), n_fix))
        for i in frames:
            for j in frames:
                seen[i, j] = True
    s = Set(W, poses, facs, W)
    zeros = (int((~seen).sum()), int((~seen.diagonal()).sum()))
    _subset_rule(ctx, "d W %d sparse" % W, s, zeros)
    # one frame empty in every factor: its block row, block column and gradient slice are exactly 0.0
    e = W // 2
    counts = [0 if i == e else 25 + 3 * i for i in range(W)]
    s = Set(W, poses, [fr.plane_factor(rng, true, counts, 20 * (k % 2)) for k in range(6)], W)
    out, _ = _subset_rule(ctx, "d W %d frame %d empty" % (W, e), s, (2 * W - 1, 1))
    assert np.all(out["H"][6 * e: 6 * e + 6, :] == 0.0) and np.all(out["H"][:, 6 * e: 6 * e + 6] == 0.0)
    assert np.all(out["g"][6 * e: 6 * e + 6] == 0.0)


# ---- e. indexing ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", WINS)
def test_indexing(oracle_lib, ctx_for, W):
    ctx = ctx_for(W)
    rng = np.random.default_rng(3000 + W)
    true, poses = fr.window(rng, W)
    s = Set(W, poses, [fr.plane_factor(rng, true, n_fix=20 * (k % 2)) for k in range(6)], W)
    assert all(len(set(c[:, 12].tolist())) == W for c, _ in s.factors)  # every frame's N differs
    base, e_orc = _subset_rule(ctx, "e W %d" % W, s)
    # the ring: frame i's cluster in slot (i + r) mod W; the logical inputs are the same, so is every bit
    for r in sorted({1, W - 1}):
        o = _run(ctx, s, ring=(np.arange(W) + r) % W)
        assert _same(base, o), r
    # fac_node: node ids with gaps, neither contiguous nor sorted, with other clusters on the nodes beside them
    ids = rng.permutation(5000)[:6] * 2 + 100
    assert sorted(ids.tolist()) != ids.tolist()
    decoy = fr.plane_factor(rng, true)
    o = _run(ctx, s, node_ids=ids, decoys=(np.r_[ids + 1, ids - 1], decoy))
    assert _same(base, o)
    o = _run(ctx, s, node_ids=ids, ring=(np.arange(W) + 1) % W, decoys=(np.r_[ids + 1, ids - 1], decoy))
    assert _same(base, o)
    # the factor order: per-factor outputs follow it bit for bit, the sums move within the bounds
    order = np.array([4, 2, 5, 0, 3, 1])
    out, _ = _subset_rule(ctx, "e W %d shuffled" % W, s, order=order, node_ids=ids)
    assert np.array_equal(out["eig"], base["eig"][order]) and np.array_equal(out["pcr"], base["pcr"][order])
    # a longer set across chunk boundaries, shuffled, against the oracle
    g = _generic(W)
    n = hess_fs(W) + 9
    order = rng.permutation(n)
    ids = rng.permutation(4000)[:n] + 7
    a, b = _run(ctx, g, n), _run(ctx, g, n, order=order, node_ids=ids, ring=(np.arange(W) + W - 1) % W)
    assert np.array_equal(b["eig"], a["eig"][order]) and np.array_equal(b["pcr"], a["pcr"][order])
    _full_rule(ctx, "e W %d nf %d shuffled" % (W, n), W, {**b, "eig": a["eig"], "pcr": a["pcr"]}, n)
    _check_resid("e W %d nf %d shuffled" % (W, n), b)


# ---- f. conditioning -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", WINS)
def test_conditioning(oracle_lib, ctx_for, W):
    ctx = ctx_for(W)
    rng = np.random.default_rng(4000 + W)
    true, poses = fr.window(rng, W, perturb=1e-6)
    for ratio in (1e3, 2.0, 1 + 1e-3):
        s = Set(W, poses, [fr.gap_factor(rng, true, ratio, n_fix=20 * k) for k in range(2)], W)
        _subset_rule(ctx, "f W %d gap %.4g" % (W, ratio), s)
    true, poses = fr.window(rng, W)
    s = Set(W, poses, [fr.plane_factor(rng, true, n_fix=20 * k, centre=c)
                       for k, c in enumerate(([300.0, -400.0, 10.0], [-353.0, 353.0, -20.0]))], W)
    _subset_rule(ctx, "f W %d 500 m" % W, s)


# ---- arguments -----------------------------------------------------------------------------------------------

def test_arguments_are_checked(ctx_for):
    W = 3
    ctx, s = ctx_for(W), _generic(3)
    c, f = s.factors[0]
    clus, fix = fr.to_dev(c)[None], fr.to_dev(f)[None]
    ring = np.arange(W)
    ok = ctx.ba_factors(W, [5], [5], clus, fix, s.xs, ring)
    assert ok["res"] > 0.0
    cap_f = max(100_000 // 8, 4096)  # ba_alloc's factor capacity for this context's max_nodes
    for fac_node, nodes, kw in (([0] * (cap_f + 1), [0], {}),  # more factors than ba.cap_f
                                ([100_000], [100_000], {}),     # a node past the map's capacity
                                ([-1], [-1], {}),
                                ([6], [5], {}),                 # a factor on a node the call does not write
                                ([5], [5], {"G": HESS_GRID_MAX + 1}), ([5], [5], {"nrb": RESID_BLOCKS + 1}),
                                ([5], [5], {"G": -1}), ([5], [5], {"nrb": -1})):
        with pytest.raises(vgpu.VgError):
            ctx.ba_factors(W, fac_node, nodes, clus, fix, s.xs, ring, **kw)
    with pytest.raises(vgpu.VgError):
        ctx.ba_factors(W, [5], [5], clus, fix, s.xs, [0, 1, 3])
    assert _same(ok, ctx.ba_factors(W, [5], [5], clus, fix, s.xs, ring))


# ---- the fused residual + Hessian pass at the other windows -----------------------------------------------------

@pytest.mark.parametrize("W", [8, 9, 11])
def test_resid_hess_equals_separate_passes(W):
    """test_stage_api_gpu.py's test_fused_launches_equal_separate for knob 34 (k_ba_resid_hess against
    k_ba_resid + k_ba_hess) at the windows beside the bench's 10 that take the fused pass
    (resid_hess_ok: W >= 8), on the 16-line sequence over W + 4 scans."""
    p = vgconfig.load("mid360")
    p["LocalBA"]["win_size"] = W
    g = p["General"]
    seq = synth.Sequence("16line", 7, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    cap = dict(max_points=120_000, max_nodes=600_000, max_fix_points=2_000_000, hash_log2=20)
    a, b = vgpu.Context(vgconfig.to_c(p), **cap), vgpu.Context(vgconfig.to_c(p), **cap)
    try:
        for c, kv in ((a, {14: 2, 34: 0}), (b, {14: 2})):
            for key, val in kv.items():
                assert vgpu.lib().vgx_debug(c.h, key, val) == 0
        a.seed(seq.gt_state(0))
        b.seed(seq.gt_state(0))
        lm = 0
        for k in range(W + 4):
            xyz, it, beg, end = seq.scan(k)
            imu = seq.imu(k)
            a.step(xyz, it, beg, end, imu)
            b.step(xyz, it, beg, end, imu)
            sa, sb = a.stats(), b.stats()
            assert sa == sb, (k, sa, sb)
            lm += sb["ba_iters"] > 0 and sb["n_factors"] > 0
        assert lm > 0
        assert np.array_equal(a.trajectory(), b.trajectory())
        assert np.array_equal(a.window_states(), b.window_states())
    finally:
        a.close()
        b.close()
