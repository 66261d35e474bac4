"""NumPy / Python-int restatement of the local-moments semantics (DESIGN.md §4 "Local moments"): the oracle of the tests.

Queries X (n, 3) and targets Y (m, 3) are (z, y, x) float32.  Target j is in the neighbourhood of
query i iff both rows are finite and nearest_ref's float32 predicate holds.  With
xq = trunc(ldexp(x, q_a)) and dq = yq - xq, a query's ten words are the count, the three sums of
dq and the six sums of dq_a dq_b (zz, zy, zx, yy, yx, xx) over its neighbourhood.

``brute`` evaluates that with Python integers from explicit float32 blocks of the (n, m) predicate
matrix; ``cells`` restates the kernel's route -- the keys of both clouds in one box, the 27 cells
around a query -- and must give the same words.  ``planes`` solves a row's plane from the exact
integer numerator of its covariance and ``np.linalg.eigh``.
"""
import math

import numpy as np

import nearest_ref as N

WORDS = 10
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))       # zz, zy, zx, yy, yx, xx
Q_MIN, Q_MAX, QBITS = -126, 62, 25
SNAP = 2.0 ** -30          # a unit normal's component this small counts as 0 in the sign rule (rounding noise around 0)


def fixed(X, q):
    """trunc(ldexp(x, q_a)) per axis -> int64 (n, 3); 0 for a non-finite row."""
    X = np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(X.shape, dtype=np.int64)
    fin = np.isfinite(X).all(axis=1)
    for a in range(3):
        out[fin, a] = np.trunc(np.ldexp(X[fin, a], np.int32(q[a])).astype(np.float64)).astype(np.int64)
    return out


def row_words(d):
    """d: int64 (k, 3) offsets of one neighbourhood -> its ten words as Python ints."""
    d = d.astype(object)
    w = [int(d.shape[0])] + [int(d[:, a].sum()) if d.shape[0] else 0 for a in range(3)]
    return w + [int((d[:, a] * d[:, b]).sum()) if d.shape[0] else 0 for a, b in PAIRS]


def brute(X, Y, r, q, rows=512):
    """-> (words: object array (n, 10) of Python ints, skipped, skipped_targets)."""
    X = np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3)
    Y = np.ascontiguousarray(Y, dtype=np.float32).reshape(-1, 3)
    n, m = X.shape[0], Y.shape[0]
    _, r2 = N.radius2(r)
    finx, finy = np.isfinite(X).all(axis=1), np.isfinite(Y).all(axis=1)
    xq, yq = fixed(X, q), fixed(Y, q)
    words = np.zeros((n, WORDS), dtype=object)
    if m:
        for a in range(0, n, rows):
            b = min(n, a + rows)
            with np.errstate(invalid="ignore"):
                near = (N.sqdist_block(X[a:b], Y) <= r2) & finx[a:b, None] & finy[None, :]
            for i in range(a, b):
                words[i] = row_words(yq[near[i - a]] - xq[i])
    return words, int(n - finx.sum()), int(m - finy.sum())


def as_int64(words):
    """The words as the int64 array the kernel writes (asserts that they fit)."""
    assert all(-(1 << 63) <= int(v) < 1 << 63 for v in words.ravel())
    return words.astype(np.int64)


def cells(X, Y, r, q):
    """The words by the kernel's route: sort the targets by key, scan the 27 cells around each query -> (words, s)."""
    X = np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3)
    Y = np.ascontiguousarray(Y, dtype=np.float32).reshape(-1, 3)
    n = X.shape[0]
    _, r2 = N.radius2(r)
    s, clo = N.plan(X, Y, r)
    kx, ky = N.keys(X, s, clo), N.keys(Y, s, clo)
    order = np.argsort(ky, kind="stable")
    nvt = int(np.isfinite(Y).all(axis=1).sum())
    sk, rows = ky[order][:nvt], order[:nvt]
    Ys, yqs, xq = Y[rows], fixed(Y, q)[rows], fixed(X, q)
    words = np.zeros((n, WORDS), dtype=object)
    mask21 = (1 << N.AXIS_BITS) - 1
    for i in np.flatnonzero(np.isfinite(X).all(axis=1)):
        cz, cy, cx = kx[i] >> 2 * N.AXIS_BITS, (kx[i] >> N.AXIS_BITS) & mask21, kx[i] & mask21
        parts = []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                zc, yc = cz + dz, cy + dy
                if not (0 <= zc <= mask21 and 0 <= yc <= mask21):
                    continue
                base = ((zc << N.AXIS_BITS) | yc) << N.AXIS_BITS
                a = np.searchsorted(sk, base + max(cx - 1, 0), side="left")
                b = np.searchsorted(sk, base + min(cx + 1, mask21), side="right")
                if b > a:
                    ok = N.sqdist_block(X[i:i + 1], Ys[a:b])[0] <= r2
                    parts.append(yqs[a:b][ok] - xq[i])
        if parts:
            words[i] = row_words(np.concatenate(parts))
    return words, s


# ---------------------------------------------------------------- the exponents
def bound(r, q):
    """B = floor(float64(float32(r)) (1 + 2^-20) 2^q) + 1, exactly."""
    v = float(np.float32(r)) * (1.0 + 2.0 ** -20)              # one float64 rounding, as the wrapper's
    num, den = v.as_integer_ratio()
    return (num << q) // den + 1 if q >= 0 else num // (den << -q) + 1


def qcap(m, r):
    rows = max(int(m), 1)
    return max(q for q in range(Q_MIN, Q_MAX + 1) if rows * bound(r, q) ** 2 <= 1 << 62 and bound(r, q) < 1 << 31)


def maxabs(X, Y):
    U = np.concatenate([np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3),
                        np.ascontiguousarray(Y, dtype=np.float32).reshape(-1, 3)])
    F = U[np.isfinite(U).all(axis=1)]
    return np.abs(F).max(axis=0).astype(np.float64) if F.shape[0] else np.zeros(3)


def default_q(X, Y, r):
    """min(fixed_q(max|.| over both clouds)[a], qcap) with fixed_q = 25 - e, max|.| < 2^e."""
    cap = qcap(np.asarray(Y).reshape(-1, 3).shape[0], r)
    return tuple(min(QBITS - (0 if v == 0 else math.frexp(float(v))[1]), cap) for v in maxabs(X, Y))


def max_offset(X, Y, r, q):
    """max |dq_a| per axis over the pairs the predicate admits -> int64[3] (0 when there is none)."""
    X = np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3)
    Y = np.ascontiguousarray(Y, dtype=np.float32).reshape(-1, 3)
    _, r2 = N.radius2(r)
    xq, yq = fixed(X, q), fixed(Y, q)
    fin = np.isfinite(Y).all(axis=1)
    out = np.zeros(3, dtype=np.int64)
    for i in np.flatnonzero(np.isfinite(X).all(axis=1)):
        near = (N.sqdist_block(X[i:i + 1], Y)[0] <= r2) & fin
        if near.any():
            out = np.maximum(out, np.abs(yq[near] - xq[i]).max(axis=0))
    return out


# ---------------------------------------------------------------- the planes
def covariance(words, q):
    """-> (cov float64 (n, 3, 3), mu float64 (n, 3)): the integer numerator c M_ab - S_a S_b divided once by c^2."""
    n = len(words)
    cov, mu = np.full((n, 3, 3), np.nan), np.full((n, 3), np.nan)
    for i in range(n):
        w = [int(v) for v in words[i]]
        c = w[0]
        if c < 1:
            continue
        for a in range(3):
            mu[i, a] = math.ldexp(w[1 + a] / c, -q[a])             # int / int: correctly rounded
        for k, (a, b) in enumerate(PAIRS):
            cov[i, a, b] = cov[i, b, a] = math.ldexp((c * w[4 + k] - w[1 + a] * w[1 + b]) / (c * c), -(q[a] + q[b]))
    return cov, mu


def planes(words, q, min_count=3):
    """-> dict(normal (n, 3), distance, roughness, planarity, lam (n, 3) ascending, cov, mu), float64; NaN where
    count < max(min_count, 1)."""
    n = len(words)
    cov, mu = covariance(words, q)
    out = dict(normal=np.full((n, 3), np.nan), distance=np.full(n, np.nan), roughness=np.full(n, np.nan),
               planarity=np.full(n, np.nan), lam=np.full((n, 3), np.nan), cov=cov, mu=mu)
    for i in range(n):
        if int(words[i][0]) < max(int(min_count), 1):
            continue
        lam, vec = np.linalg.eigh(cov[i])
        v = np.where(np.abs(vec[:, 0]) <= SNAP, 0.0, vec[:, 0])    # a component within 2^-30 of 0 is 0: noise picks no sign
        if v[0] < 0 or (v[0] == 0 and (v[1] < 0 or (v[1] == 0 and v[2] < 0))):
            v = -v
        out["normal"][i], out["lam"][i] = v, lam
        out["distance"][i] = -float(v @ mu[i])
        out["roughness"][i] = math.sqrt(max(lam[0], 0.0))
        out["planarity"][i] = (lam[1] - lam[0]) / lam[2] if lam[2] > 0 else 0.0
    return out


# ---------------------------------------------------------------- the clouds of the tests
def raster_days(h=37, w=150, seed=8):
    """Three days of one h x w raster surface, each with its own speckle far off the surface
    (the cloud of the support tests, restated)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    clouds, groups = [], []
    for g in range(3):
        z = 3.0 * np.sin(xx / 23.0) + 2.0 * np.cos(yy / 7.0) + 0.2 * rng.standard_normal(xx.shape)
        c = np.stack([z, yy, xx], axis=-1).reshape(-1, 3)[rng.random(h * w) < 0.5]
        k = 20
        speckle = np.stack([rng.uniform(8, 30, k) * rng.choice([-1, 1], k), rng.uniform(0, h, k), rng.uniform(0, w, k)], 1)
        clouds.append(np.concatenate([c, speckle]).astype(np.float32))
        groups.append(np.full(clouds[-1].shape[0], g))
    return clouds, np.concatenate(groups)


def clump_cloud():
    """The first 2000 rows of the raster cloud and two clumps of 100 duplicates each, 2.4 apart along x."""
    base = np.concatenate(raster_days()[0])[:2000]
    a = np.float32([40.0, 18.0, 200.0])                        # off the raster: the clumps see only each other
    b = a + np.float32([0.0, 0.0, 2.4])
    return np.concatenate([base, np.tile(a, (100, 1)), np.tile(b, (100, 1))]).astype(np.float32)
