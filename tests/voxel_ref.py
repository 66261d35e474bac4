"""NumPy restatement of the voxel semantics (DESIGN.md §4 "Voxels"): the oracle of the tests.

Rows are (z, y, x) float32.  On axis a the cell of a finite row is, in float32 with every
operation rounded,

    c_a = floor((x_a - o_a) * inv_a),   inv_a = float32(1.0 / float64(v_a)).

A row with a NaN or Inf coordinate belongs to no voxel.  The occupied voxels come in ascending
(cz, cy, cx) order; per voxel the count, the exact sums of trunc(ldexp(x_a, q_a)), the lowest row
and the mask of the groups seen.
"""
import math

import numpy as np

QBITS = 25
AXIS_BITS = 21
CELL_ABS_MAX = np.float32(2.0 ** 40)


def sizes(voxel):
    """-> (float32 sizes (3,), float32 inverses (3,))."""
    v = np.asarray(voxel, dtype=np.float64).astype(np.float32)
    if v.shape == ():
        v = np.full(3, v, dtype=np.float32)
    assert v.shape == (3,) and np.isfinite(v).all() and (v > 0).all()
    return v, (1.0 / v.astype(np.float64)).astype(np.float32)


def cellf(x, o, inv):
    """floor((x - o) * inv), every operation a rounded float32 operation."""
    x, o, inv = (np.asarray(t, dtype=np.float32) for t in (x, o, inv))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        d = (x - o).astype(np.float32)
        return np.floor((d * inv).astype(np.float32)).astype(np.float32)


def fixed_q(maxabs):
    return [QBITS - (0 if float(m) == 0.0 else math.frexp(float(m))[1]) for m in maxabs]


def plan(F, o, inv, voxel):
    """The corner check over the finite rows F (at least one) -> the low corner's cell, int64 (3,)."""
    lo, hi = cellf(F.min(axis=0), o, inv), cellf(F.max(axis=0), o, inv)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError(f"voxel={voxel!r}: a cell index of the bounding box is not finite")
    if (np.abs(lo) > CELL_ABS_MAX).any() or (np.abs(hi) > CELL_ABS_MAX).any():
        raise ValueError(f"voxel={voxel!r}: a cell index exceeds 2^40")
    span = hi.astype(np.int64) - lo.astype(np.int64) + 1
    if (span > 1 << AXIS_BITS).any() or (span == 1 << AXIS_BITS).all():
        raise ValueError(f"voxel={voxel!r}: an axis spans more than 2^21 cells")
    return lo.astype(np.int64)


def voxel_grid(X, voxel, origin=(0.0, 0.0, 0.0), groups=None, q=None):
    """-> dict(cells, counts, sums, first, day_mask (None without groups), inverse, skipped, q, inv, order)
    with the dtypes of the product; ``order``: the finite rows sorted by (voxel, row)."""
    X = np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3)
    n = X.shape[0]
    v, inv = sizes(voxel)
    o = np.asarray(origin, dtype=np.float64).astype(np.float32)
    fin = np.isfinite(X).all(axis=1)
    rows = np.flatnonzero(fin)
    F = X[rows]
    if q is None:
        q = fixed_q(np.abs(F).max(axis=0)) if rows.size else [QBITS] * 3
    q = [int(t) for t in q]
    inverse = np.full(n, -1, dtype=np.int32)
    out = dict(skipped=int(n - rows.size), q=q, inv=inv, inverse=inverse, order=np.zeros(0, dtype=np.int64))
    if not rows.size:
        out.update(cells=np.zeros((0, 3), np.int64), counts=np.zeros(0, np.int32), sums=np.zeros((0, 3), np.int64),
                   first=np.zeros(0, np.int32), day_mask=None if groups is None else np.zeros(0, np.int64))
        return out
    plan(F, o, inv, voxel)
    c = cellf(F, o, inv).astype(np.int64)                                   # (nf, 3)
    order = np.lexsort((rows, c[:, 2], c[:, 1], c[:, 0]))                   # by cz, cy, cx, then row
    cs = c[order]
    head = np.ones(rows.size, dtype=bool)
    head[1:] = (cs[1:] != cs[:-1]).any(axis=1)
    seg = np.cumsum(head) - 1
    M = int(seg[-1]) + 1
    inverse[rows[order]] = seg.astype(np.int32)
    xq = np.trunc(np.ldexp(F[order], np.asarray(q, dtype=np.int32))).astype(np.int64)
    sums = np.zeros((M, 3), dtype=np.int64)
    np.add.at(sums, seg, xq)
    first = np.full(M, np.iinfo(np.int32).max, dtype=np.int64)
    np.minimum.at(first, seg, rows[order])
    day_mask = None
    if groups is not None:
        g = np.asarray(groups).astype(np.int64)[rows[order]]
        assert ((g >= 0) & (g < 64)).all()
        m = np.zeros(M, dtype=np.uint64)
        np.bitwise_or.at(m, seg, np.uint64(1) << g.astype(np.uint64))
        day_mask = m.view(np.int64)
    out.update(cells=cs[head], counts=np.bincount(seg, minlength=M).astype(np.int32), sums=sums,
               first=first.astype(np.int32), day_mask=day_mask, order=rows[order])
    return out


def centroids(ref):
    """float32 of (float64(S) * 2^-q) / float64(count)."""
    scale = np.ldexp(1.0, -np.asarray(ref["q"], dtype=np.int64))
    return ((ref["sums"].astype(np.float64) * scale) / ref["counts"].astype(np.float64)[:, None]).astype(np.float32)


def days(ref):
    return np.array([bin(int(m) & (2 ** 64 - 1)).count("1") for m in ref["day_mask"]], dtype=np.int32)


def downsample(X, voxel, mode="centroid", origin=(0.0, 0.0, 0.0), min_count=1, min_days=1, groups=None):
    """-> (points float32 (M', 3), rows int32 (M',), the voxel_grid dict)."""
    X = np.ascontiguousarray(X, dtype=np.float32).reshape(-1, 3)
    ref = voxel_grid(X, voxel, origin, groups)
    keep = ref["counts"] >= min_count
    if min_days > 1:
        keep &= days(ref) >= min_days
    rows = ref["first"][keep]
    return (centroids(ref)[keep] if mode == "centroid" else X[rows]), rows, ref


def thin(X, voxel):
    """The plugin's ``voxels=`` stand-in: (X float32 (n, 3), (vz, vy, vx)) -> (points, counts, inverse)."""
    pts, _, ref = downsample(X, voxel)
    return pts, ref["counts"], ref["inverse"]


# ---------------------------------------------------------------- the clouds of the tests
def lattice_cloud(n=4000, seed=3):
    """Coordinates integers(-64, 64) / 4: exact in float32, many exactly on the faces of voxels of
    size 0.5, 1 or 2, on both sides of 0 (floor, not trunc)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-64, 64, size=(n, 3)).astype(np.float64) / 4.0).astype(np.float32)


def face_cloud(n=3000, seed=4):
    """General floats around 0 plus points exactly on faces (multiples of 0.25 and of 0.3f), -0.0 and
    duplicates."""
    rng = np.random.default_rng(seed)
    a = (rng.random((n, 3)) * np.array([4.0, 12.0, 12.0]) - np.array([2.0, 5.0, 7.0])).astype(np.float32)
    b = (rng.integers(-20, 20, size=(n // 3, 3)) * 0.25).astype(np.float32)
    c = (rng.integers(-20, 20, size=(n // 3, 3)).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    z = np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, -0.0, -0.0]], dtype=np.float32)
    X = np.concatenate([a, b, c, z, a[:50]])
    return X[rng.permutation(X.shape[0])]


def edge_cloud(seed=5):
    """A shuffled cloud on the integer line x = 0, 1, 2, ... (voxel 1) whose voxel populations are
    [60, 8, 120, 1, 1, 66, 256, 513, 63, 64, 65, 127, 128, 129, 255, 256, 257, 3*256 + 5, ...]: in
    sorted order segments start, end and span at the boundaries of waves (64 rows) and blocks (256)."""
    pops = [60, 8, 120, 1, 1, 66, 256, 513, 63, 64, 65, 127, 128, 129, 255, 256, 257, 3 * 256 + 5, 2, 62, 64, 64, 1, 191,
            64, 3]
    rng = np.random.default_rng(seed)
    x = np.repeat(np.arange(len(pops), dtype=np.float32), pops)
    X = np.stack([rng.random(x.size).astype(np.float32) * np.float32(0.5), np.full(x.size, 0.25, dtype=np.float32),
                  x + np.float32(0.5)], axis=1)
    dup = np.flatnonzero(x == pops.index(3 * 256 + 5))
    X[dup] = X[dup[0]]                                                  # 3*256 + 5 duplicates of one point
    return X[rng.permutation(x.size)], pops
