"""CPU tests of tests/kpp_geometry.py, the NumPy restatement of the k-means++
pruning grid: the thin-box table (which boxes exceed the workspace bound before
the clamp), the clamp's postcondition over a sweep of extents, and
``step_branches`` against the oracle it follows."""
import itertools

import numpy as np
import pytest

import kpp_geometry as KG
from oracle import kpp_ref as P
from oracle import lloyd_ref as R

# n, extents, G of make_grid, its cells, kpp_cells_max
TABLE = [
    (150_000, (30, 1800, 2400), (1, 30, 40), 1200, 1980),
    (150_000, (5, 1800, 2400), (1, 54, 72), 3888, 1980),
    (150_000, (2, 1800, 2400), (1, 73, 98), 7154, 1980),
    (4_300_000, (2, 1800, 2400), (1, 225, 300), 67_500, 56_692),
    (10_800, (1, 90, 120), (1, 14, 19), 266, 145),
    (25_600, (1, 1, 1000), (1, 1, 464), 464, 340),
    (20_000, (0.001, 1), (1, 280), 280, 178),
]


@pytest.mark.parametrize("n,ext,G,cells,bound", TABLE, ids=[f"n{r[0]}-{'x'.join(map(str, r[1]))}" for r in TABLE])
def test_thin_box_table(n, ext, G, cells, bound):
    g = KG.make_grid(ext, KG.kpp_target(n))
    assert tuple(g.G) == G and g.ncells == cells
    assert KG.kpp_cells_max(n, len(ext)) == bound
    before = list(g.G)
    KG.clamp_grid(g, bound)
    assert 1 <= g.ncells <= bound
    if cells <= bound:
        assert g.G == before                      # a grid that fits is left as make_grid made it
    else:
        assert g.G != before and g.G[0] == 1


def test_predict_thin_shapes_exceed_the_bound():
    """Every thin cloud of the predict tests overflows the k-means++ bound before the clamp."""
    got = {}
    for n, _, ext in KG.THIN:
        g = KG.make_grid(ext, KG.kpp_target(n))
        bound = KG.kpp_cells_max(n, len(ext))
        assert g.ncells > bound, (n, ext, g.G, bound)
        got[(n, ext)] = (g.ncells, bound)
        assert 1 <= KG.clamp_grid(g, bound).ncells <= bound
    assert got[(1000, (1, 1e-4, 1))] == (1156, 16)
    assert got[(50_001, (1, 1e-6, 1))] == (336_400, 662)


def test_thin_list_is_the_predict_tests():
    pytest.importorskip("torch")
    import test_gpu_predict as TP
    assert KG.THIN == TP.THIN


EXTS = (1e-6, 1e-3, 1.0, 1e3, 1e6)
NS = (1, 2, 255, 256, 257, 1000, 10_800, 150_000, 5_000_000)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_clamp_postcondition_sweep(d):
    """1 <= ncells <= kpp_cells_max after the clamp; axes stay within [1, 4096]; a grid
    that fits is unchanged; constant axes keep one cell."""
    rng = np.random.default_rng(d)
    boxes = list(itertools.product(EXTS, repeat=d))
    boxes += [tuple(10.0 ** rng.uniform(-6, 6, d)) for _ in range(300)]
    boxes += [tuple(0.0 if a == z else e for a, e in enumerate(b)) for b in boxes[:25] for z in range(d)]
    for n in NS:
        bound = KG.kpp_cells_max(n, d)
        for ext in boxes:
            g = KG.make_grid(ext, KG.kpp_target(n))
            before, fits = list(g.G), g.ncells <= bound
            KG.clamp_grid(g, bound)
            assert 1 <= g.ncells <= bound, (n, ext, g.G)
            assert all(1 <= v <= 4096 for v in g.G)
            assert all(v == 1 for v, e in zip(g.G, ext) if e == 0.0)
            assert fits == (g.G == before)
            for a in range(d):
                assert g.w[a] * g.G[a] == pytest.approx(ext[a]) and (g.inv[a] > 0) == (ext[a] > 0)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_cube_shaped_clouds_never_clamp(d):
    """Equal extents: make_grid's rounding stays inside 1.5**d * target, so the benchmark's grid is unchanged."""
    for n in (1, 300, 20_000, 1_000_000, 12_500_000, 100_000_000):
        g = KG.make_grid((7.0,) * d, KG.kpp_target(n))
        assert g.ncells <= KG.kpp_cells_max(n, d), (n, d, g.G)


def test_cube_clamps_and_whole_axes():
    g = KG.Grid((-1.0, 0.0, 0.0), (2.0, 100.0, 100.0), (1, 20, 20))
    assert g.ncells == 400 and g.w[1] == 5.0
    i0, i1, vol = KG.kpp_cube(g, (0.0, 50.0, 50.0), np.float32(0.0))       # gmax 0: one cell of slack each way
    assert (i0, i1, vol) == ([0, 9, 9], [0, 11, 11], 9)
    i0, i1, vol = KG.kpp_cube(g, (0.0, 0.0, 100.0), np.float32(36.0))      # corners clamp to the grid
    assert (i0, i1, vol) == ([0, 0, 17], [0, 2, 19], 9)
    assert KG.kpp_cube(g, (0.0, 50.0, 50.0), np.float32(1e6))[2] == g.ncells


@pytest.mark.parametrize("n,k,d,seed,L", [(3000, 20, 2, 7, None), (5000, 16, 4, 11, 16), (2500, 12, 1, 5, 1),
                                          (4000, 70, 3, 2, 9)])
def test_step_branches_follows_the_oracle(n, k, d, seed, L):
    X = R.splitmix_uniform(n, d, seed=seed + 100)
    idx, steps = KG.step_branches(X, k, seed, L)
    np.testing.assert_array_equal(idx, P.kmeanspp(X, k, seed, L)[1])
    assert [s["c"] for s in steps] == list(range(1, k))
    assert steps[-1]["dense"] is None and all(s["dense"] is not None for s in steps[:-1])
    c = KG.branch_counts(steps)
    if L == 1:
        assert c["early"] == 0            # one cube alone never holds more items than the grid has cells
    assert c["early"] + c["late"] == k - 1 and c["dense"] + c["sparse"] == k - 2
    assert c["late_at_c64"] <= max(0, k - 64)


def test_crafted_stream_and_zero_potential():
    """The crafted stream is consumed alike by both sides; the oracle's picks once the potential is 0."""
    from pcm_amd import kpp as K
    cyc = [0.0, 1.0 - 2.0 ** -53, 0.5, 0.25, 2.0 ** -53]
    u0, um = K._draws(KG.CraftedState(0.0, cyc), 4, 5)
    v0, us = P.draws(KG.CraftedState(0.0, cyc), 4, 5)
    assert u0 == v0 == 0.0
    np.testing.assert_array_equal(um, np.ldexp(us.ravel(), 53).astype(np.uint64))
    np.testing.assert_array_equal(us[0], cyc)
    assert P.first_index(4097, 0.0) == 0 and P.first_index(4097, 1.0 - 2.0 ** -53) == 4096
    rng = np.random.default_rng(5)
    base = rng.uniform(-3, 3, (12, 3)).astype(np.float32)
    X = np.repeat(base, 400, axis=0)[rng.permutation(4800)]
    _, idx = P.kmeanspp(X, 20, 3)
    assert len({X[i].tobytes() for i in idx[:12]}) == 12 and (idx[12:] == 0).all()
    _, idx = P.kmeanspp(np.tile(base[:1], (500, 1)), 5, 3)
    assert (idx[1:] == 0).all()
