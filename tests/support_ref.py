"""NumPy restatement of the support semantics (DESIGN.md §4 "Support"): the oracle of the tests.

Rows are (z, y, x) float32.  With r2 = float32(r) * float32(r), row j is a neighbour of row i
(j != i) iff, in float32 with every operation rounded,

    dz = z_i - z_j; dy = y_i - y_j; dx = x_i - x_j;   (dz*dz + dy*dy) + dx*dx <= r2.

``brute`` evaluates that on an explicit (n, n) float32 matrix; ``cells`` restates the kernel's
route -- the cell exponent, the keys, the 27 cells around a row -- and must give the same counts.
"""
import math

import numpy as np

S_MIN = -32
AXIS_BITS = 21
CELL_ABS_MAX = np.float32(2.0 ** 40)


def predicate(X, r):
    """The (n, n) bool matrix of the float32 predicate, the diagonal and non-finite rows cleared."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    r = np.float32(r)
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = np.float32(r * r)
        d = X[:, None, :] - X[None, :, :]                       # float32
        sq = d * d
        d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        near = d2 <= r2
    fin = np.isfinite(X).all(axis=1)
    near &= fin[:, None] & fin[None, :]
    np.fill_diagonal(near, False)
    return near


def brute(X, r, groups=None, n_groups=None, max_count=None):
    """-> (counts int32 (n,), days int32 (n,) or None, skipped)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0]
    near = predicate(X, r)
    fin = np.isfinite(X).all(axis=1)
    counts = near.sum(axis=1).astype(np.int64)
    if max_count is not None:
        counts = np.minimum(counts, max_count)
    days = None
    if groups is not None:
        groups = np.asarray(groups).astype(np.int64)
        G = int(n_groups) if n_groups is not None else (int(groups.max()) + 1 if n else 1)
        own = near | (np.eye(n, dtype=bool) & fin[:, None])
        seen = np.zeros((n, G), dtype=bool)
        for g in range(G):
            seen[:, g] = own[:, groups == g].any(axis=1)
        days = seen.sum(axis=1).astype(np.int32)
    return counts.astype(np.int32), days, int(n - fin.sum())


def keep_mask(X, r, min_neighbors=1, min_days=1, groups=None, n_groups=None):
    counts, days, _ = brute(X, r, groups, n_groups)
    keep = (counts >= min_neighbors) & np.isfinite(np.asarray(X, dtype=np.float32)).all(axis=1)
    if days is not None:
        keep &= days >= min_days
    return keep


# ---------------------------------------------------------------- the cells
def radius_exponent(r) -> int:
    """The smallest s with 2^s >= float32(r) * (1 + 2^-20), at least S_MIN."""
    m, e = math.frexp(float(np.float32(r)) * (1.0 + 2.0 ** -20))     # m in [0.5, 1)
    return max(e - 1 if m == 0.5 else e, S_MIN)


def cellf(x, s):
    """floor(ldexp(x, -s)) in float32."""
    with np.errstate(over="ignore", under="ignore"):
        return np.floor(np.ldexp(np.asarray(x, dtype=np.float32), np.int32(-s))).astype(np.float32)


def plan(X, r):
    """-> (s, clo int64[3], bits[3]): the cell exponent, the cell of the low corner, the bits per axis."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    s = radius_exponent(r)
    F = X[np.isfinite(X).all(axis=1)]
    if not F.shape[0]:
        return s, np.zeros(3, dtype=np.int64), [0, 0, 0]
    lo, hi = F.min(axis=0), F.max(axis=0)
    m = np.float32(max(np.abs(lo).max(), np.abs(hi).max()))
    while not cellf_scale(m, s) <= CELL_ABS_MAX:
        s += 1
    while True:
        clo = cellf(lo, s).astype(np.int64)
        span = cellf(hi, s).astype(np.int64) - clo + 1
        if (span <= 1 << AXIS_BITS).all():
            return s, clo, [int(v - 1).bit_length() for v in span]
        s += 1


def cellf_scale(m, s):
    with np.errstate(over="ignore"):
        return np.ldexp(np.float32(m), np.int32(-s))


def keys(X, r):
    """-> (keys int64 (n,), s): (cz << 42) | (cy << 21) | cx, 2^63 - 1 for a non-finite row."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    s, clo, _ = plan(X, r)
    fin = np.isfinite(X).all(axis=1)
    c = np.zeros(X.shape, dtype=np.int64)
    c[fin] = cellf(X[fin], s).astype(np.int64) - clo
    assert (c >= 0).all() and (c < 1 << AXIS_BITS).all()
    k = (c[:, 0] << 2 * AXIS_BITS) | (c[:, 1] << AXIS_BITS) | c[:, 2]
    k[~fin] = np.iinfo(np.int64).max
    return k, s


def cells(X, r, max_count=None):
    """The counts by the kernel's route: sort by key, scan the 27 cells around each row."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0]
    k, s = keys(X, r)
    order = np.argsort(k, kind="stable")
    sk = k[order]
    nv = int(np.isfinite(X).all(axis=1).sum())
    sk = sk[:nv]
    Xs = X[order[:nv]]
    r2 = np.float32(np.float32(r) * np.float32(r))
    counts = np.zeros(n, dtype=np.int64)
    mask21 = (1 << AXIS_BITS) - 1
    for i in range(nv):
        cz, cy, cx = sk[i] >> 2 * AXIS_BITS, (sk[i] >> AXIS_BITS) & mask21, sk[i] & mask21
        total = 0
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                zc, yc = cz + dz, cy + dy
                if not (0 <= zc <= mask21 and 0 <= yc <= mask21):
                    continue
                base = ((zc << AXIS_BITS) | yc) << AXIS_BITS
                a = np.searchsorted(sk, base + max(cx - 1, 0), side="left")
                b = np.searchsorted(sk, base + min(cx + 1, mask21), side="right")
                if b > a:
                    with np.errstate(over="ignore", invalid="ignore"):
                        d = Xs[i][None, :] - Xs[a:b]
                        sq = d * d
                        d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
                        total += int((d2 <= r2).sum()) - (1 if a <= i < b else 0)
        counts[order[i]] = total
    if max_count is not None:
        counts = np.minimum(counts, max_count)
    return counts.astype(np.int32), s


# ---------------------------------------------------------------- the clouds of the tests
def lattice_cloud(n=3000, seed=5):
    """Coordinates integers(-128, 128) / 4 with z further scaled by 1/4: squared distances are
    exact in float32 and in float64."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-128, 128, size=(n, 3)).astype(np.float64) / 4.0
    X[:, 0] /= 4.0
    return X.astype(np.float32)


def face_cloud(r):
    """Pairs at exactly r across a cell face on each axis, across an edge and across a corner
    (3-4-5 and 2-3-6-7 style offsets scaled to r), on both sides of 0 and at multiples of 2^s;
    then pairs just inside and outside, and the pair (2^s, -2^-30 2^s) whose true gap exceeds a
    power-of-two r though its float32 difference equals it."""
    s = radius_exponent(r)
    side = 2.0 ** s
    r = float(np.float32(r))
    pts = []
    for base in (0.0, side, -side, 3 * side, -4 * side):
        for a in range(3):                                   # a face
            p = np.full(3, base)
            q = p.copy()
            q[a] -= r
            pts += [p, q]
            q = p.copy()
            q[a] += r * (1 + 2.0 ** -20)                     # outside
            pts.append(q)
        for a, b in ((0, 1), (0, 2), (1, 2)):                # an edge: 3-4-5
            p = np.full(3, base)
            q = p.copy()
            q[a] -= 0.6 * r
            q[b] -= 0.8 * r
            pts += [q]
            q = p.copy()
            q[a] += 0.6 * r
            q[b] -= 0.8 * r
            pts += [q]
        for sz, sy, sx in ((1, 1, 1), (-1, 1, -1), (-1, -1, -1)):     # a corner: 2-3-6-7
            q = np.full(3, base) + np.array([sz * 2, sy * 3, sx * 6]) * (r / 7.0)
            pts.append(q)
    X = np.asarray(pts, dtype=np.float32)
    tiny = np.float32(-side * 2.0 ** -30)
    far = 200 * side
    extra = np.array([[far, 0, tiny], [far, 0, r], [far, tiny, far], [far, r, far], [tiny, far, 0], [r, far, 0]],
                     dtype=np.float32)
    return np.concatenate([X, extra, -extra])
