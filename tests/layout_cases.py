"""Inputs of the layout tests (TEST INFRASTRUCTURE ONLY; NumPy only).

One list of named cases serves tests/test_layout_ref.py (which asserts, from tests/layout_ref.py
alone, that every case reaches the edge it is named for) and tests/test_gpu_layout_edges.py (the
built layout against tests/layout_ref.py).  ``build(name)`` gives a case: the cloud ``X``, the
number of centres ``k`` (it decides sub-cells, label width and the crowded-cell test, nothing
else here) and ``env``, the values of PCM_CELL_TARGET, PCM_TILE_CAP and PCM_ZLEV the layout is
built under (``pcm_layout_build`` reads them at every layout).

Families: ``edge-*`` sizes on the wave and chunk edges of the sort; ``vec-*`` the 16-byte row
loads' tails; ``pass-*`` key widths of 1 to 4 passes; ``seg-*`` the segment scan; ``skew-*`` digit
histograms a ranking scatter can get wrong; ``tiles-*`` cell counts on the tile bounds; ``xz-*``
the compression decision; ``crowd-*`` Morton-ordered cells.
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import layout_ref as LR

DTYPES = {"f32": np.float32, "f16": np.float16}
# PCM_CELL_TARGET of the edge family by d (K = 32 keeps the sub-cells of d <= 3): 9- and 10-bit keys, two
# passes with position maps
EDGE_TARGET = {1: "200", 2: "100", 3: "64", 4: "512"}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _case(name, X, k, env, dtype=None):
    X = np.ascontiguousarray(X, dtype=DTYPES[dtype] if dtype else X.dtype)
    assert X.ndim == 2 and np.isfinite(X.astype(np.float32)).all()
    X.setflags(write=False)
    return SimpleNamespace(name=name, X=X, n=X.shape[0], d=X.shape[1], k=int(k), env=dict(env),
                           dtype={np.dtype(np.float32): "f32", np.dtype(np.float16): "f16"}[X.dtype])


def edge_sizes(ch):
    return (1, 3, 4, 5, 63, 64, 65, 511, 512, 513, ch - 1, ch, ch + 1, 2 * ch + 1)


def edge_names():
    out = []
    for dt, d in (("f32", 3), ("f32", 4), ("f16", 3)):
        out += [f"edge-{dt}d{d}-n{n}" for n in edge_sizes(LR.chunk_items(DTYPES[dt], d))]
    for dt, d in (("f32", 1), ("f32", 2), ("f16", 1), ("f16", 4)):
        out.append(f"edge-{dt}d{d}-n{LR.chunk_items(DTYPES[dt], d) + 1}")
    return out


def vec_names():
    return [f"vec-n{4 * 4096 + r}" for r in range(4)]


PASS_BITS = (8, 9, 16, 17, 21, 32)
SEG_NAMES = ("seg-f32d3-n1048575", "seg-f32d3-n1048577", "seg-f32d4-n786433", "seg-f32d1-n8388613")
SKEW_NAMES = ("skew-onecell", "skew-constant", "skew-alternate", "skew-sorted", "skew-reverse", "skew-dups",
              "skew-faces", "skew-digit255")
TILE_NAMES = ("tiles-cap512", "tiles-default", "tiles-onecell")
XZ_NAMES = ("xz-widths", "xz-neg", "xz-straddle", "xz-zeros")
CROWD_NAMES = ("crowd-auto", "crowd-z1-f16d2", "crowd-z3", "crowd-z6")


def pass_names():
    return [f"pass-b{b}" for b in PASS_BITS]


def names():
    """Every case but the million-point ones (SEG_NAMES: the GPU test takes them one by one)."""
    return (edge_names() + vec_names() + pass_names() + list(SKEW_NAMES) + list(TILE_NAMES) + list(XZ_NAMES)
            + list(CROWD_NAMES))


def _uniform(rng, n, d, dtype, lo=0.0, hi=1.0):
    return rng.uniform(lo, hi, (n, d)).astype(DTYPES[dtype])


def _in_cells(rng, counts, G, width=1.0):
    """counts[c] points strictly inside cell c (row-major over G) of the grid of cell size `width` at 0."""
    rows = []
    for c, m in enumerate(counts):
        idx = np.unravel_index(c, G)
        rows.append((np.asarray(idx)[None, :] + rng.uniform(0.05, 0.95, (m, len(G)))) * width)
    X = np.concatenate(rows)
    return X[rng.permutation(len(X))]


def _tiles_cloud(rng, cap):
    """A 4 x 2 x 2 grid over [0, 4] x [0, 2] x [0, 2] whose cells hold 0, 1, cap, cap + 1, 2 cap and
    2 cap + 1 points (and counts beside them); the last cell is empty.  The four box corners that fix
    the grid lie in cells (0,0,0), (3,0,0), (0,1,0) and (0,0,1) and count towards those."""
    G = (4, 2, 2)
    counts = [cap, cap + 1, 3, 2 * cap, 2, 2 * cap + 1, 0, cap - 1, 1, 5, cap + 2, 7, cap + 1, 2 * cap + 1, 6, 0]
    corners = {(0, 0, 0): (0.0, 0.0, 0.0), (3, 0, 0): (4.0, 0.0, 0.0), (0, 1, 0): (0.0, 2.0, 0.0),
               (0, 0, 1): (0.0, 0.0, 2.0)}
    inner = list(counts)
    for idx in corners:
        inner[int(np.ravel_multi_index(idx, G))] -= 1
    X = np.concatenate([_in_cells(rng, inner, G), np.asarray(list(corners.values()))])
    return X[rng.permutation(len(X))].astype(np.float32), counts


def _ulps(base, m):
    """fp32 values whose bit patterns are base's plus m."""
    return (np.asarray(m, np.int64) + int(np.float32(base).view(np.uint32))).astype(np.uint32).view(np.float32)


def _xz_widths(rng):
    """[1, 2]^3 in 2 x 2 x 2 cells (patterns 0x3f800000 + m, m <= 2^23; a cell spans 2^22 of them):
    cell (0,0,0) spans 22 + 21 + 21 = 64 bits (compressed), cell (1,0,0) 22 + 22 + 21 = 65 (raw), cell
    (0,1,0) holds one point, cell (0,0,1) has constant y and z, cell (1,1,0) constant x, cell (1,1,1)
    the far corner."""
    H = 1 << 22

    def cell(ix, iy, iz, sx, sy, sz, m=40):
        """m points of cell (ix, iy, iz) whose patterns span exactly [0, s] past the cell's corner per axis."""
        cols = []
        for i, s in zip((ix, iy, iz), (sx, sy, sz)):
            v = rng.integers(0, s + 1, m)
            v[0], v[1] = 0, s
            cols.append(_ulps(1.0, i * H + v[rng.permutation(m)]))
        return np.stack(cols, 1)
    rows = [cell(0, 0, 0, (1 << 21) + 5, (1 << 20) + 9, (1 << 21) - 1),        # widths 22, 21, 21
            cell(1, 0, 0, (1 << 21) + 5, (1 << 21), (1 << 21) - 1),            # 22, 22, 21
            cell(0, 1, 0, 0, 0, 0, m=2)[:1],                                   # one point
            cell(0, 0, 1, 1 << 15, 0, 0),                                      # y, z constant: widths 16, 0, 0 -> 1
            cell(1, 1, 0, 0, 1 << 10, 1 << 12),                                # x constant
            cell(1, 1, 1, 77, 99, 1 << 20),
            np.asarray([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0]], np.float32)]
    X = np.concatenate(rows)
    return X[rng.permutation(len(X))]


@functools.lru_cache(maxsize=8)
def build(name):
    rng = _rng(name)
    fam, *rest = name.split("-")
    if fam == "edge":                                       # edge-<dtype>d<d>-n<n>
        dt, d = rest[0][:3], int(rest[0][4:])
        return _case(name, _uniform(rng, int(rest[1][1:]), d, dt), 32, {"PCM_CELL_TARGET": EDGE_TARGET[d]})
    if fam == "vec":
        return _case(name, _uniform(rng, int(rest[0][1:]), 3, "f32"), 32, {"PCM_CELL_TARGET": "64"})
    if fam == "pass":
        bits = int(rest[0][1:])
        if bits == 8:                                       # 3^3 cells << 3 sub-cell bits
            return _case(name, _uniform(rng, 20000, 3, "f32"), 8, {"PCM_CELL_TARGET": "27"})
        if bits == 9:                                       # 4^3 << 3: widths 5, 4
            return _case(name, _uniform(rng, 20000, 3, "f32"), 32, {"PCM_CELL_TARGET": "64"})
        if bits == 16:                                      # 40^3 = 64000 cells, no sub-cells: 8, 8
            return _case(name, _uniform(rng, 30000, 3, "f32"), 8, {"PCM_CELL_TARGET": "64000"})
        if bits == 17:                                      # 46^3 = 97336 cells: 6, 6, 5
            return _case(name, _uniform(rng, 30000, 3, "f32"), 8, {"PCM_CELL_TARGET": "100000"})
        if bits == 21:                                      # 64^3 cells << 3 (K > ncells / 8 keeps the sub-cells): 7, 7, 7
            return _case(name, _uniform(rng, 50000, 3, "f32"), 40000, {"PCM_CELL_TARGET": "262144"})
        if bits == 32:                                      # a flat box: 1024 x 1024 x 1 cells, 4 Morton levels: 4 x 8
            X = _uniform(rng, 30000, 3, "f32")
            X[:, 2] *= np.float32(1e-6)
            return _case(name, X, 8, {"PCM_CELL_TARGET": "262144", "PCM_ZLEV": "4"})
    if fam == "seg":                                        # the box's extremes in the last two rows
        dt, d, n = rest[0][:3], int(rest[0][4:]), int(rest[1][1:])
        X = _uniform(rng, n, d, dt, 0.125, 0.875)
        X[n - 2], X[n - 1] = 0.0, 1.0
        return _case(name, X, 8, {"PCM_CELL_TARGET": "4096"})
    if fam == "skew":
        kind, n, env = rest[0], 3 * 4096 + 77, {"PCM_CELL_TARGET": "64"}
        X = _uniform(rng, n, 3, "f32")
        if kind == "onecell":                               # two corners fix the box, the rest in one cell
            X = (0.55 + 0.1 * X).astype(np.float32)
            X[17], X[n - 5] = 0.0, 1.0
        elif kind == "constant":
            X[:] = np.float32(0.375)
        elif kind == "alternate":                           # rows alternate between the first and the last cell
            X = (0.2 * X).astype(np.float32)
            X[1::2] += np.float32(0.75)
            X[0], X[1] = 0.0, 1.0
        elif kind in ("sorted", "reverse"):
            p = LR.plan(X, 32, env)
            order = np.argsort(LR.sort_keys(X, p.g, p.sub, p.zlev), kind="stable")
            X = X[order if kind == "sorted" else order[::-1]]
        elif kind == "dups":                                # 4096 copies of one row among the others
            X[rng.choice(n, 4096, replace=False)] = X[0]
        elif kind == "faces":                               # multiples of 1/8: cell faces, half-cell splits, the top face
            X = (rng.integers(0, 9, (n, 3)) / 8.0).astype(np.float32)
            X[0], X[1] = 0.0, 1.0
        elif kind == "digit255":                            # 256 x 256 cells, 8 + 8 bits; 40 % of the rows on the top faces
            X = (rng.integers(0, 257, (n, 2)) / 256.0).astype(np.float32)
            X[rng.random(n) < 0.4] = 1.0
            X[rng.random(n) < 0.2, 0] = 1.0
            X[0], X[1] = 0.0, 1.0
            env = {"PCM_CELL_TARGET": "65536"}
        return _case(name, X, 32, env)
    if fam == "tiles":
        if rest[0] == "onecell":                            # one cell of 2 cap + 1 points: three tiles
            return _case(name, _uniform(rng, 2 * 512 + 1, 3, "f32"), 8, {"PCM_CELL_TARGET": "1", "PCM_TILE_CAP": "512"})
        cap = 512 if rest[0] == "cap512" else LR.TILE
        X, _ = _tiles_cloud(rng, cap)
        return _case(name, X, 8, {"PCM_CELL_TARGET": "16", **({"PCM_TILE_CAP": "512"} if cap == 512 else {})})
    if fam == "xz":
        kind = rest[0]
        if kind == "widths":
            return _case(name, _xz_widths(rng), 8, {"PCM_CELL_TARGET": "8"})
        if kind == "neg":
            return _case(name, _uniform(rng, 20000, 3, "f32", -2.0, -1.0), 8, {"PCM_CELL_TARGET": "64"})
        if kind == "straddle":                              # cells next to 0 hold both signs; those far from it compress
            return _case(name, _uniform(rng, 30000, 3, "f32", -1.2, 2.8), 8, {"PCM_CELL_TARGET": "512"})
        if kind == "zeros":                                 # x, y and a third of z within 1023 patterns of 1.0 (tiles that
            m = rng.integers(0, 1024, (6000, 3))            # compress); the other rows' z is +0.0 or -0.0, in one tile
            m[0], m[1] = 0, 1023
            X = _ulps(1.0, m)
            X[2::3, 2] = 0.0
            X[3::3, 2] = -0.0
            return _case(name, X, 8, {"PCM_CELL_TARGET": "8"})
    if fam == "crowd":
        kind = rest[0]
        if kind == "auto":                                  # 3000 of 4000 points in one cell: the sample decides
            X = _uniform(rng, 4000, 3, "f32")
            X[500:3500] = (0.6 + 0.05 * X[500:3500]).astype(np.float32)
            return _case(name, X, 96, {"PCM_CELL_TARGET": "64", "PCM_TILE_CAP": "512"})
        if kind == "z1":
            X = _uniform(rng, 9000, 2, "f16")
            return _case(name, X, 8, {"PCM_CELL_TARGET": "16", "PCM_TILE_CAP": "512", "PCM_ZLEV": "1"})
        X = _uniform(rng, 20000, 3, "f32")
        X[::2] = (0.3 + 0.1 * X[::2]).astype(np.float32)
        return _case(name, X, 8, {"PCM_CELL_TARGET": "64", "PCM_TILE_CAP": "512", "PCM_ZLEV": kind[1:]})
    raise KeyError(name)
