"""NumPy reference of ``pcm_align_stats`` / ``pcm_align_apply`` and of the registration driver,
built on the oracle's canonical E-step and fixed point (oracle.lloyd_ref: assign, sqdist_rows,
to_fixed).  ``encode`` forms the 38 words per group with ``np.add.at`` on uint64 and the kernel's
limb split; ``direct`` forms the same sums in Python ints; ``register`` is the product's driver
loop (``pcm_amd.align.register_loop``: the host code is the same) over ``encode``.
"""
import os

import numpy as np

from oracle import lloyd_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align", "recovery_k256.npz")

WORDS = 38
QBITS = 25
MASK = (1 << 32) - 1


def transform(X, T=None, groups=None):
    """p_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a in float32, every operation rounded; T None: p = x.
    Rows whose group has no transform come back NaN (pcm_align_apply)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if T is None:
        return X.copy()
    T = np.asarray(T, dtype=np.float32).reshape(-1, 12)
    g = np.zeros(X.shape[0], dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    known = g < T.shape[0]
    Tg = T[np.where(known, g, 0)]
    P = np.empty_like(X)
    with np.errstate(all="ignore"):
        for a in range(3):
            m0, m1, m2 = Tg[:, 3 * a] * X[:, 0], Tg[:, 3 * a + 1] * X[:, 1], Tg[:, 3 * a + 2] * X[:, 2]
            P[:, a] = ((m0 + m1) + m2) + Tg[:, 9 + a]
    P[~known] = np.nan
    return P


def rows(X, C, groups, G, T, max_d2, q):
    """Per row: (group, valid, inlier, pq (n, 3) int64, cq (n, 3) int64)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    C = np.ascontiguousarray(C, dtype=np.float32)
    q = np.asarray(q, dtype=np.int32)
    n = X.shape[0]
    g = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    with np.errstate(all="ignore"):
        valid = np.isfinite(X).all(1) & (g < G)
        gs = np.where(valid, g, 0)
        P = transform(np.where(valid[:, None], X, np.float32(0)), T, gs if T is not None else None)
        valid &= np.isfinite(P).all(1)
        valid &= (np.abs(np.ldexp(P, q[None, :])) < np.float32(1 << QBITS)).all(1)
    P = np.where(valid[:, None], P, np.float32(0))
    j = R.assign(P, C) if n else np.zeros(0, dtype=np.int32)
    with np.errstate(over="ignore"):
        d2 = R.sqdist_rows(P, C[j]) if n else np.zeros(0, dtype=np.float32)
        inl = valid & (d2 <= np.float32(max_d2))
    return g, valid, inl, R.to_fixed(P, q), R.to_fixed(C[j], q)


def _values(pq, cq):
    """(m, 36) int64: word 0 and words 2..37 of one row each (word 1 is the outlier count)."""
    cols = [np.ones(pq.shape[0], dtype=np.int64)] + [pq[:, a] for a in range(3)] + [cq[:, a] for a in range(3)]
    prods = [pq[:, a] * cq[:, b] for a in range(3) for b in range(3)] + [pq[:, a] * pq[:, a] for a in range(3)] + \
            [cq[:, a] * cq[:, a] for a in range(3)]
    for p in prods:
        cols += [p & MASK, p >> 32]
    return np.stack(cols, axis=1)


def encode(X, C, q, groups=None, G=1, T=None, max_d2=np.inf):
    """-> (words uint64 (G, 38), skipped)."""
    g, valid, inl, pq, cq = rows(X, C, groups, G, T, max_d2, q)
    words = np.zeros((G, WORDS), dtype=np.uint64)
    out = valid & ~inl
    np.add.at(words[:, 1], g[out], np.uint64(1))
    vals = _values(pq[inl], cq[inl]).view(np.uint64)
    cols = [0] + list(range(2, WORDS))
    with np.errstate(over="ignore"):
        for i, w in enumerate(cols):
            np.add.at(words[:, w], g[inl], vals[:, i])
    return words, int((~valid).sum())


def direct(X, C, q, groups=None, G=1, T=None, max_d2=np.inf):
    """The same sums in Python ints: per group dict(inliers, outliers, sp, sc, cross, sqp, sqc)."""
    g, valid, inl, pq, cq = rows(X, C, groups, G, T, max_d2, q)
    res = [dict(inliers=0, outliers=0, sp=[0] * 3, sc=[0] * 3, cross=[[0] * 3 for _ in range(3)], sqp=[0] * 3,
                sqc=[0] * 3) for _ in range(G)]
    for i in np.flatnonzero(valid):
        r = res[int(g[i])]
        if not inl[i]:
            r["outliers"] += 1
            continue
        r["inliers"] += 1
        p, c = [int(v) for v in pq[i]], [int(v) for v in cq[i]]
        for a in range(3):
            r["sp"][a] += p[a]
            r["sc"][a] += c[a]
            r["sqp"][a] += p[a] * p[a]
            r["sqc"][a] += c[a] * c[a]
            for b in range(3):
                r["cross"][a][b] += p[a] * c[b]
    return res, int((~valid).sum())


def stats_of(X, C, groups, G, T, max_dist):
    """The AlignStats of ``encode`` with the product's default exponents (align.default_q)."""
    from pcm_amd import align
    X = np.ascontiguousarray(X, dtype=np.float32)
    C = np.ascontiguousarray(C, dtype=np.float32)
    q = align.default_q(np.abs(X).max(0) if X.shape[0] else np.zeros(3), np.abs(C).max(0), T)
    words, skipped = encode(X, C, q, groups, G, T, align._max_d2(max_dist))
    if skipped:
        raise ValueError(f"skipped {skipped} rows")
    return align.AlignStats(words, q)


def half_diagonal(C):
    C = np.asarray(C, dtype=np.float32)
    return 0.5 * float(np.linalg.norm(C.max(0).astype(np.float64) - C.min(0).astype(np.float64)))


def register(X, C, groups=None, G=1, kind="rigid", max_dist=None, max_iter=50, tol=1e-3, init=None):
    """``register_days`` with ``encode`` as the pass."""
    from pcm_amd import align
    return align.register_loop(lambda T: stats_of(X, C, groups, G, T, max_dist), G, half_diagonal(C), kind=kind,
                               max_iter=max_iter, tol=tol, init=init)


# ---------------------------------------------------------------- the recovery case
_CASE = {}


def recovery_days():
    """Two days of one terrain: a 240 x 240 raster (z = relief + 0.3 noise, 90 % of the pixels kept,
    each day its own noise and mask), float64 (z, y, x)."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:240, 0:240].astype(np.float64)
    relief = 9.0 * np.sin(yy / 17.0) * np.cos(xx / 23.0) + 6.0 * np.cos((yy + 2.0 * xx) / 31.0) + \
        8.0 * ((yy > 60) & (yy < 110) & (xx > 130) & (xx < 190)) + 5.0 * ((yy - 170) ** 2 + (xx - 60) ** 2 < 900)

    def day():
        keep = rng.random(relief.shape) < 0.9
        z = relief + rng.normal(0.0, 0.3, relief.shape)
        return np.stack([z[keep], yy[keep], xx[keep]], axis=1)

    return day(), day()


def recovery_case():
    """The two days of ``recovery_days``, the converged Lloyd centres of day 0 at K = 256 (the golden
    file tests/golden/align/make_align_golden.py writes: a model that has not converged biases the
    registration by the distance of its centres from their cells' centroids), and day 1 displaced by
    0.4 degrees about the axis (0.3, 1, 0.2) through its centroid plus t = (-1.3, 1.7, -2.2).
    -> dict(X (n, 3) float32 both days, groups, C, true1 (day 1 undisplaced), rms0 (the displacement's rms))."""
    if _CASE:
        return _CASE
    d0, d1 = recovery_days()
    ax = np.array([0.3, 1.0, 0.2]) / np.linalg.norm([0.3, 1.0, 0.2])
    th = np.deg2rad(0.4)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rot = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    cen = d1.mean(0)
    moved = (d1 - cen) @ Rot.T + cen + np.array([-1.3, 1.7, -2.2])
    X0 = d0.astype(np.float32)
    with np.load(GOLDEN) as f:
        C = np.ascontiguousarray(f["centers"], dtype=np.float32)
        assert int(f["n_points"]) == X0.shape[0], "the terrain differs from the one the golden centres were fitted on"
    _CASE.update(X=np.concatenate([X0, moved.astype(np.float32)]),
                 groups=np.r_[np.zeros(len(d0), np.uint8), np.ones(len(d1), np.uint8)], C=C, true1=d1, n0=len(d0),
                 rms0=float(np.sqrt(((moved - d1) ** 2).sum(1).mean())))
    return _CASE


def point_error(X1_registered, case):
    """rms distance of day 1's registered points to where they truly lie."""
    return float(np.sqrt(((np.asarray(X1_registered, dtype=np.float64) - case["true1"]) ** 2).sum(1).mean()))


def recovery_reference():
    """``register`` of day 1 of the recovery case onto the centres (rigid, no trimming), computed once."""
    case = recovery_case()
    if "ref" not in case:
        X1 = case["X"][case["n0"]:]
        case["ref"] = register(X1, case["C"], None, 1, kind="rigid")
        case["ref_error"] = point_error(transform(X1, case["ref"].transforms), case)
    return case["ref"], case["ref_error"]


# ---------------------------------------------------------------- plugin stand-ins
def ref_align(X, C, groups, G, kind, max_dist):
    """The plugin's ``align=`` stand-in: ``register`` and ``transform`` -> (registration dict, registered X)."""
    reg = register(X, C, groups, G, kind=kind, max_dist=max_dist)
    return reg.as_dict(), transform(X, reg.transforms, groups)


def two_days(n=4000, seed=21):
    """Two small clouds of one surface (float64 z, y, x), the second tilted by 0.5 degrees about y and shifted."""
    rng = np.random.default_rng(seed)

    def day():
        yx = rng.random((n, 2)) * 60
        z = 4.0 * np.sin(yx[:, 0] / 7.0) * np.cos(yx[:, 1] / 9.0) + 3.0 * (yx[:, 0] > 30) + rng.normal(0, 0.1, n)
        return np.column_stack([z, yx])

    d0, d1 = day(), day()
    th = np.deg2rad(0.5)
    Rot = np.array([[np.cos(th), 0, -np.sin(th)], [0, 1, 0], [np.sin(th), 0, np.cos(th)]])
    cen = d1.mean(0)
    return [d0, (d1 - cen) @ Rot.T + cen + np.array([1.5, -0.6, 0.8])]
