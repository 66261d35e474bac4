"""NumPy restatement of the k-means++ pruning-grid geometry (TEST INFRASTRUCTURE ONLY).

Restates, from csrc/pcm_layout.hip, csrc/pcm_kpp.hip and csrc/pcm_kpp.hpp:

* ``make_grid``: cells sized from the box volume (``llround`` per axis, at most
  4096 cells per axis, the largest axis halved while the grid exceeds 2**20 cells);
* ``kpp_cells_max``: the cell count ``kpp_layout`` sizes the workspace for;
* ``clamp_grid``: the thin-box clamp (the axis with the most cells halved until the grid fits);
* ``kpp_cube``: the cell-index cube of half-width ``sqrt(gmax)`` around a candidate.

``step_branches`` follows ``oracle/kpp_ref.kmeanspp`` step by step (same draws,
weights, targets and first argmin) and reports, per centre, which branch the
kernels take: the eval regime, the dense or sparse apply, the late-step grid.
The tests use it to show that a cloud reaches the branch it is named for.
"""
import math

import numpy as np

from oracle import kpp_ref as P
from oracle.lloyd_ref import as_f32_points, sqdist_rows

KPP_CELL_PTS = 256
KPP_LATE_C = 64

# the thin clouds of tests/test_gpu_predict.py (n, k, per-axis extents)
THIN = [
    (1000, 8, (1, 1e-4, 1)),
    (50_001, 32, (1, 1e-6, 1)),
    (3, 2, (1000, 1, 0.001)),
    (2000, 8, (100, 0.001)),
    (100, 8, (1, 1, 1, 1e-5)),
    (20_000, 64, (1, 1, 1e-5, 1)),
    (5000, 16, (1e-3, 50)),
]


class CraftedState(np.random.RandomState):
    """A RandomState whose ``random_sample`` and ``uniform(size=...)`` hand out chosen
    values (multiples of 2**-53 in [0, 1)): ``first`` once, then ``cycle`` over and over.
    ``kpp._draws`` and ``kpp_ref.draws`` both accept it and consume the same sequence."""

    def __init__(self, first, cycle):
        super().__init__(0)
        self._first, self._cycle, self._pos = float(first), [float(v) for v in cycle], -1
        for v in [self._first] + self._cycle:
            assert 0.0 <= v < 1.0 and math.ldexp(v, 53) == int(math.ldexp(v, 53))

    def _take(self, m):
        out = np.empty(m, np.float64)
        for i in range(m):
            out[i] = self._first if self._pos < 0 else self._cycle[self._pos % len(self._cycle)]
            self._pos += 1
        return out

    def random_sample(self, size=None):
        if size is None:
            return float(self._take(1)[0])
        return self._take(int(np.prod(size))).reshape(size)

    def uniform(self, low=0.0, high=1.0, size=None):
        assert low == 0.0 and high == 1.0
        return self.random_sample(size)


def _llround(x: float) -> int:
    """C llround for x >= 0: halves away from zero (x - floor(x) is exact)."""
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


class Grid:
    """The fields of the C ``Grid`` the k-means++ kernels read."""

    def __init__(self, lo, ext, G):
        self.lo = [float(v) for v in lo]
        self.ext = [float(v) for v in ext]
        self.G = [int(v) for v in G]
        self.derive()

    def derive(self):
        self.w = [e / g for e, g in zip(self.ext, self.G)]
        self.inv = [g / e if e > 0 else 0.0 for e, g in zip(self.ext, self.G)]
        self.ncells = math.prod(self.G)


def make_grid(ext, target, lo=None) -> Grid:
    """pcm::make_grid over a box of per-axis extents ``ext`` (lower corner ``lo``, default 0)."""
    ext = [float(e) for e in ext]
    d = len(ext)
    target = max(1.0, min(float(target), float(1 << 18)))
    G = [1] * d
    nondeg = [a for a in range(d) if ext[a] > 0]
    if nondeg:
        vol = 1.0
        for a in nondeg:
            vol *= ext[a]
        sz = math.pow(vol / target, 1.0 / len(nondeg))
        for a in nondeg:
            G[a] = max(1, min(_llround(ext[a] / sz), 4096))
    while math.prod(G) > (1 << 20):
        amax = max(range(d), key=lambda a: (G[a], -a))      # the first axis with the most cells
        G[amax] = max(1, G[amax] // 2)
    return Grid([0.0] * d if lo is None else lo, ext, G)


def kpp_target(n: int) -> float:
    return max(1.0, n / KPP_CELL_PTS)


def kpp_cells_max(n: int, d: int) -> int:
    return min(1 << 20, math.ceil(math.pow(1.5, d) * kpp_target(n)) + 2)


def clamp_grid(g: Grid, ncells_max: int) -> Grid:
    """pcm::clamp_grid: a grid that fits is left alone."""
    while g.ncells > ncells_max:
        amax = max(range(len(g.G)), key=lambda a: (g.G[a], -a))
        if g.G[amax] <= 1:
            break
        g.G[amax] = max(1, g.G[amax] // 2)
        g.derive()
    return g


def kpp_grid(X, clamp=True) -> Grid:
    """The grid pcm_kmeanspp lays X out in: make_grid over the float32 bounding box, then the clamp."""
    X = as_f32_points(X)
    n, d = X.shape
    lo = X.min(axis=0).astype(np.float64)
    hi = X.max(axis=0).astype(np.float64)
    g = make_grid(hi - lo, kpp_target(n), lo)
    return clamp_grid(g, kpp_cells_max(n, d)) if clamp else g


def kpp_cube(g: Grid, c, gmax):
    """Inclusive cell ranges (i0, i1) per axis and the cell count of the cube around point c."""
    R = math.sqrt(float(np.float32(gmax)) * (1.0 + 2.0 ** -16) + 1e-36)
    i0, i1, vol = [], [], 1
    for a, G in enumerate(g.G):
        if G <= 1 or not g.inv[a] > 0.0:
            lo_i, hi_i = 0, G - 1
        else:
            ca = float(np.float32(c[a]))
            lo = math.floor((ca - R - g.lo[a]) * g.inv[a]) - 1.0
            hi = math.floor((ca + R - g.lo[a]) * g.inv[a]) + 1.0
            lo_i = 0 if lo < 0.0 else (G - 1 if lo > G - 1 else int(lo))
            hi_i = 0 if hi < 0.0 else (G - 1 if hi > G - 1 else int(hi))
        i0.append(lo_i)
        i1.append(hi_i)
        vol *= hi_i - lo_i + 1
    return i0, i1, vol


def step_branches(X, k, seed, n_local_trials=None):
    """oracle/kpp_ref.kmeanspp step by step; returns (indices, steps).

    ``steps[c - 1]`` for centre c = 1 .. k-1: ``early`` (k_kpp_eval walks whole
    cells: the candidates' cubes together hold more items than the grid has
    cells), ``dense`` (k_kpp_apply rebuilds the rows by a streaming pass; None
    for the last centre, which is not applied) and ``late_grid`` (c >= 64: the
    quarter grid of k_kpp_apply).  gmax is the largest closest distance at the
    start of the step: the cell maxima the kernels keep are exact.
    """
    X = as_f32_points(X)
    n, d = X.shape
    L = P.n_trials(k) if n_local_trials is None else int(n_local_trials)
    g = kpp_grid(X)
    u0, us = P.draws(seed, k, L)
    s = P.kpp_scale(n, P.max_dist_bound(X))
    idx = np.full(k, -1, dtype=np.int64)
    idx[0] = P.first_index(n, u0, X.dtype)
    closest = sqdist_rows(X, np.broadcast_to(X[idx[0]], X.shape))
    pot = int(P.weights(closest, s).sum(dtype=np.uint64))
    steps = []
    for c in range(1, k):
        gmax = closest.max()
        cum = np.cumsum(P.weights(closest, s), dtype=np.uint64)
        tg = np.array([P.target(u, pot) for u in us[c - 1]], dtype=np.uint64)
        cand = np.minimum(np.searchsorted(cum, tg, side="left"), n - 1)
        total = sum(kpp_cube(g, X[ci], gmax)[2] for ci in cand)
        best_pot, best_l, best_m = None, -1, None
        for l, ci in enumerate(cand):
            m = np.minimum(closest, sqdist_rows(X, np.broadcast_to(X[ci], X.shape)))
            pl = int(P.weights(m, s).sum(dtype=np.uint64))
            if best_pot is None or pl < best_pot:
                best_pot, best_l, best_m = pl, l, m
        idx[c] = cand[best_l]
        vol = kpp_cube(g, X[idx[c]], gmax)[2]
        steps.append({"c": c, "early": total > g.ncells,
                      "dense": (8 * vol >= 7 * g.ncells) if c + 1 < k else None,
                      "late_grid": c >= KPP_LATE_C})
        pot, closest = best_pot, best_m
    return idx, steps


def branch_counts(steps):
    """The step counts the tests assert on."""
    return {
        "early": sum(s["early"] for s in steps),
        "late": sum(not s["early"] for s in steps),
        "dense": sum(s["dense"] is True for s in steps),
        "sparse": sum(s["dense"] is False for s in steps),
        "late_at_c64": sum((not s["early"]) and s["late_grid"] for s in steps),
        "sparse_at_c64": sum(s["dense"] is False and s["late_grid"] for s in steps),
    }
