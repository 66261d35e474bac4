"""NumPy restatement of the nearest-point semantics (DESIGN.md §4 "Nearest"): the oracle of the tests.

Queries X (n, 3) and targets Y (m, 3) are (z, y, x) float32.  With r = float32(max_dist) and
r2 = float32(r * r), target j is a candidate of query i iff both rows are finite, their groups
(when given) differ and, in float32 with every operation rounded,

    dz = X[i,0] - Y[j,0]; dy = X[i,1] - Y[j,1]; dx = X[i,2] - Y[j,2];   d2 = (dz*dz + dy*dy) + dx*dx <= r2.

index[i] is the candidate that minimises (d2, j) -- a tie in distance goes to the LOWEST target
row --, -1 when there is none; sqdist[i] is that d2, +inf when there is none.

``brute`` evaluates that on explicit float32 blocks of the (n, m) matrix; ``cells`` restates the
kernel's route -- one cell exponent and one low corner over both clouds, the keys, the 27 cells
around a query -- and must give the same index and distance.
"""
import numpy as np

from support_ref import AXIS_BITS, CELL_ABS_MAX, cellf, cellf_scale, face_cloud, lattice_cloud, radius_exponent  # noqa: F401

INF = np.float32(np.inf)


def radius2(r):
    """-> (float32 r, float32 r*r)."""
    r = np.float32(r)
    with np.errstate(over="ignore", under="ignore"):
        return r, np.float32(r * r)


def sqdist_block(Xb, Y):
    """The (b, m) float32 matrix of d2, every operation rounded to float32, in the kernel's order."""
    with np.errstate(over="ignore", invalid="ignore"):
        dz = Xb[:, None, 0] - Y[None, :, 0]
        dy = Xb[:, None, 1] - Y[None, :, 1]
        dx = Xb[:, None, 2] - Y[None, :, 2]
        return (dz * dz + dy * dy) + dx * dx


def brute(X, Y, r, gx=None, gy=None, rows=512):
    """-> (index int32 (n,), sqdist float32 (n,), skipped, skipped_targets, tied): ``tied`` is the
    number of found rows with two or more candidates at the minimal distance."""
    X = np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3)
    Y = np.ascontiguousarray(Y, dtype=np.float32).reshape(-1, 3)
    n, m = X.shape[0], Y.shape[0]
    _, r2 = radius2(r)
    finx, finy = np.isfinite(X).all(axis=1), np.isfinite(Y).all(axis=1)
    index = np.full(n, -1, dtype=np.int32)
    sqdist = np.full(n, INF, dtype=np.float32)
    tied = 0
    if m:
        if gx is not None:
            gx, gy = np.asarray(gx).astype(np.int64), np.asarray(gy).astype(np.int64)
        for a in range(0, n, rows):
            b = min(n, a + rows)
            d2 = sqdist_block(X[a:b], Y)
            with np.errstate(invalid="ignore"):
                cand = (d2 <= r2) & finx[a:b, None] & finy[None, :]
            if gx is not None:
                cand &= gx[a:b, None] != gy[None, :]
            masked = np.where(cand, d2, INF)               # a candidate's d2 is finite: <= r2 < inf
            j = masked.argmin(axis=1)                      # the first minimum: the lowest row
            best = masked[np.arange(b - a), j]
            found = cand.any(axis=1)
            index[a:b] = np.where(found, j, -1)
            sqdist[a:b] = np.where(found, best, INF)
            tied += int((((masked == best[:, None]) & cand).sum(axis=1)[found] >= 2).sum())
    return index, sqdist, int(n - finx.sum()), int(m - finy.sum()), tied


# ---------------------------------------------------------------- the cells
def plan(X, Y, r):
    """-> (s, clo int64[3]): the cell exponent and the cell of the low corner of the box over the
    finite rows of BOTH clouds (support's rule on the union)."""
    s = radius_exponent(r)
    U = np.concatenate([np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3),
                        np.ascontiguousarray(Y, dtype=np.float32).reshape(-1, 3)])
    F = U[np.isfinite(U).all(axis=1)]
    if not F.shape[0]:
        return s, np.zeros(3, dtype=np.int64)
    lo, hi = F.min(axis=0), F.max(axis=0)
    m = np.float32(max(np.abs(lo).max(), np.abs(hi).max()))
    while not cellf_scale(m, s) <= CELL_ABS_MAX:
        s += 1
    while True:
        clo = cellf(lo, s).astype(np.int64)
        span = cellf(hi, s).astype(np.int64) - clo + 1
        if (span <= 1 << AXIS_BITS).all():
            return s, clo
        s += 1


def keys(X, s, clo):
    """-> keys int64 (n,): (cz << 42) | (cy << 21) | cx, 2^63 - 1 for a non-finite row."""
    X = np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3)
    fin = np.isfinite(X).all(axis=1)
    c = np.zeros(X.shape, dtype=np.int64)
    c[fin] = cellf(X[fin], s).astype(np.int64) - clo
    assert (c >= 0).all() and (c < 1 << AXIS_BITS).all()
    k = (c[:, 0] << 2 * AXIS_BITS) | (c[:, 1] << AXIS_BITS) | c[:, 2]
    k[~fin] = np.iinfo(np.int64).max
    return k


def cells(X, Y, r, gx=None, gy=None):
    """Index and distance by the kernel's route: sort the targets by key, scan the 27 cells
    around each query -> (index, sqdist, s)."""
    X = np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3)
    Y = np.ascontiguousarray(Y, dtype=np.float32).reshape(-1, 3)
    n, m = X.shape[0], Y.shape[0]
    _, r2 = radius2(r)
    s, clo = plan(X, Y, r)
    kx, ky = keys(X, s, clo), keys(Y, s, clo)
    order = np.argsort(ky, kind="stable")
    nvt = int(np.isfinite(Y).all(axis=1).sum())
    sk, rows = ky[order][:nvt], order[:nvt]
    Ys = Y[rows]
    if gx is not None:
        gx, gys = np.asarray(gx).astype(np.int64), np.asarray(gy).astype(np.int64)[rows]
    index = np.full(n, -1, dtype=np.int32)
    sqdist = np.full(n, INF, dtype=np.float32)
    mask21 = (1 << AXIS_BITS) - 1
    for i in np.flatnonzero(np.isfinite(X).all(axis=1)):
        cz, cy, cx = kx[i] >> 2 * AXIS_BITS, (kx[i] >> AXIS_BITS) & mask21, kx[i] & mask21
        best = (INF, -1)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                zc, yc = cz + dz, cy + dy
                if not (0 <= zc <= mask21 and 0 <= yc <= mask21):
                    continue
                base = ((zc << AXIS_BITS) | yc) << AXIS_BITS
                a = np.searchsorted(sk, base + max(cx - 1, 0), side="left")
                b = np.searchsorted(sk, base + min(cx + 1, mask21), side="right")
                if b <= a:
                    continue
                d2 = sqdist_block(X[i:i + 1], Ys[a:b])[0]
                ok = d2 <= r2
                if gx is not None:
                    ok &= gys[a:b] != gx[i]
                for t in np.flatnonzero(ok):
                    best = min(best, (d2[t], int(rows[a + t])))
        if best[1] >= 0:
            sqdist[i], index[i] = best
    return index, sqdist, s


# ---------------------------------------------------------------- the clouds of the tests
BOX = (np.array([8.0, 64.0, 64.0]), np.array([3.0, 17.0, 40.0]))


def general_clouds():
    """4096 queries and 3000 targets, general floats in one box around 0."""
    X = (np.random.default_rng(3).random((4096, 3)) * BOX[0] - BOX[1]).astype(np.float32)
    Y = (np.random.default_rng(4).random((3000, 3)) * BOX[0] - BOX[1]).astype(np.float32)
    return X, Y


def lattice_clouds():
    """Two clouds whose squared distances are exact in float32: many pairs at exactly r."""
    return lattice_cloud(3000, 5), lattice_cloud(2500, 6)


def tie_clouds():
    """Small integer coordinates: most queries have several targets at the minimal distance."""
    X = np.random.default_rng(21).integers(0, 12, (700, 3)).astype(np.float32)
    Y = np.random.default_rng(22).integers(0, 12, (600, 3)).astype(np.float32)
    return X, Y


def crowded_clouds(c, seed=None):
    """-> (X, Y, the point): Y is ``c`` copies of one point and 300 points around it, shuffled; the
    queries are that point and the 300 others."""
    rng = np.random.default_rng(c if seed is None else seed)
    point = np.float32([0.25, -0.5, 0.125])
    around = (rng.random((300, 3)) * 4.0 - 2.0).astype(np.float32)
    Y = np.concatenate([np.tile(point, (c, 1)), around])
    Y = Y[rng.permutation(Y.shape[0])]
    X = np.concatenate([point[None, :], around])
    return X, Y, point
