"""CPU: the support reference (tests/support_ref.py) pinned to scipy's cKDTree and to its own
cell restatement, the argument checks of the three entry points and of the Python layer, and the
plugin's ``denoise=`` paths through the ``support=`` stand-in (the product has no CPU fallback;
the HIP kernels are checked in tests/test_gpu_support.py).
"""
import ctypes
import os

import numpy as np
import pytest

import support_ref as S
from oracle import lloyd_ref as R

LATTICE_RADII = (0.75, 1.25, 2.5)


@pytest.fixture(scope="module")
def lattice():
    return S.lattice_cloud(3000, 5)


@pytest.fixture(scope="module")
def lattice_counts(lattice):
    return {r: S.brute(lattice, r)[0] for r in LATTICE_RADII}


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("r", LATTICE_RADII)
def test_brute_force_equals_ckdtree_on_the_lattice(lattice, lattice_counts, r):
    """Squared distances of the lattice are exact in float32 and float64, so the float64 tree
    must count what the float32 predicate counts -- and pairs at exactly r exist, so <= is pinned."""
    from scipy.spatial import cKDTree
    X64 = lattice.astype(np.float64)
    want = cKDTree(X64).query_ball_point(X64, r, return_length=True) - 1
    assert np.array_equal(lattice_counts[r], want)
    d = X64[:, None, :] - X64[None, :, :]
    ties = int(np.triu((d * d).sum(-1) == r * r, 1).sum())
    print(f"r={r}: {ties} pairs at exactly r")
    assert ties > 0


@pytest.mark.parametrize("r", LATTICE_RADII)
def test_cells_equal_brute_force_on_the_lattice(lattice, lattice_counts, r):
    got, s = S.cells(lattice, r)
    assert np.array_equal(got, lattice_counts[r])
    assert 2.0 ** s >= r > 2.0 ** (s - 1)


@pytest.mark.parametrize("r", (0.5, 1.0, 1.25, 3.0))
def test_cells_equal_brute_force_on_the_faces(r):
    X = S.face_cloud(r)
    want = S.brute(X, r)[0]
    got, s = S.cells(X, r)
    assert np.array_equal(got, want)
    # a power-of-two radius needs the next exponent: the pair (r, -2^-30 r) is a pair of neighbours
    # (their float32 difference is r) whose true gap exceeds r
    assert s == {0.5: 0, 1.0: 1, 1.25: 1, 3.0: 2}[r]
    near = S.predicate(X, r)
    d = X.astype(np.float64)[:, None, :] - X.astype(np.float64)[None, :, :]
    assert (near & ((d * d).sum(-1) == r * r)).any()                      # pairs at exactly r ...
    if r in (0.5, 1.0):
        assert (near & (np.abs(d).max(-1) > r)).any()                     # ... and the rounded one beyond it


def test_cell_exponent_rules():
    assert S.radius_exponent(1.0) == 1 and S.radius_exponent(0.99) == 0 and S.radius_exponent(1e-30) == S.S_MIN
    assert S.radius_exponent(np.nextafter(np.float32(1.0), np.float32(0))) == 1   # within 2^-20 of a power of two
    # two clumps 1e6 apart at r = 0.01: the span rule raises s from -6 until 2^21 cells cover the gap
    X = np.array([[0, 0, 0], [0, 0, 1e6]], dtype=np.float32)
    s, clo, bits = S.plan(X, 0.01)
    assert S.radius_exponent(0.01) == -6 and s == -1 and bits == [0, 0, 21]
    # far from the origin the magnitude rule keeps the cells exact integers
    s, clo, bits = S.plan(np.full((2, 3), 1e30, dtype=np.float32), 0.01)
    assert np.ldexp(np.float32(1e30), -s) <= 2.0 ** 40 < np.ldexp(np.float32(1e30), -(s - 1))
    k, _ = S.keys(np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], dtype=np.float32), 1.0)
    assert k.tolist() == [0, 2 ** 63 - 1, 2 ** 63 - 1]


def test_reference_semantics_on_a_hand_case():
    X = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, 2.5], [np.nan, 0, 0], [0, 0, np.inf]], dtype=np.float32)
    counts, days, skipped = S.brute(X, 1.0, groups=[0, 1, 2, 3, 1, 1], n_groups=4)
    assert counts.tolist() == [2, 2, 2, 0, 0, 0] and days.tolist() == [3, 3, 3, 1, 0, 0] and skipped == 2
    assert S.brute(X, 1.0, max_count=1)[0].tolist() == [1, 1, 1, 0, 0, 0]
    assert S.keep_mask(X, 1.0, 1).tolist() == [True, True, True, False, False, False]
    assert S.keep_mask(X, 1.0, 1, 4, groups=[0, 1, 2, 3, 1, 1]).tolist() == [False] * 6


# ---------------------------------------------------------------- the C ABI without a device
@pytest.fixture(scope="module")
def lib():
    from pcm_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.load(require_gpu_runtime=False)


def test_support_argument_errors_without_device(lib):
    from pcm_amd import _lib
    nbytes = ctypes.c_size_t()
    assert lib.pcm_support_workspace(-1, ctypes.byref(nbytes)) == -1
    assert "pcm_support_workspace" in _lib.last_error()
    assert lib.pcm_support_workspace(1 << 31, ctypes.byref(nbytes)) == -1
    assert lib.pcm_support_workspace(10, None) == -1
    assert lib.pcm_support_workspace(1000, ctypes.byref(nbytes)) == 0 and nbytes.value >= 1000 * 17
    f = ctypes.c_float
    assert lib.pcm_support_keys(None, -1, f(1.0), None, None, None) == -1
    assert "pcm_support_keys" in _lib.last_error() and "n must be" in _lib.last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.pcm_support_keys(None, 5, f(bad), None, None, None) == -1
        assert "radius" in _lib.last_error()
    assert lib.pcm_support_keys(None, 5, f(1.0), None, None, None) == -1          # no info block
    args = (None, None, None, None, None, None, 0, None)
    assert lib.pcm_support_count(None, -1, None, 1, f(1.0), -1, *args) == -1
    assert "pcm_support_count" in _lib.last_error()
    assert lib.pcm_support_count(None, 5, None, 1, f(0.0), -1, *args) == -1
    assert "radius" in _lib.last_error()
    for g in (0, 65):
        assert lib.pcm_support_count(None, 5, None, g, f(1.0), -1, *args) == -1
        assert "n_groups must be 1..64" in _lib.last_error()
    assert lib.pcm_support_count(None, 5, None, 1, f(1.0), -1, *args) == -1       # null pointers
    assert lib.pcm_support_count(None, 0, None, 1, f(1.0), -1, *args) == 0        # nothing to count


def test_constants_mirror_the_header():
    import re
    from pcm_amd import _lib
    src = open(os.path.join(_lib.REPO_DIR, "include", "pcm_kmeans.h")).read()
    for name, value in (("CHUNK", _lib.SUPPORT_CHUNK), ("TPB", _lib.SUPPORT_TPB), ("MAXG", _lib.SUPPORT_MAXG),
                        ("INFO_WORDS", _lib.SUPPORT_INFO_WORDS)):
        assert int(re.search(rf"#define PCM_SUPPORT_{name} (\d+)", src).group(1)) == value
    assert _lib.SUPPORT_CHUNK % 64 == 0


# ---------------------------------------------------------------- the Python layer
def test_python_validation_without_device():
    torch = pytest.importorskip("torch")
    import pcm_amd
    from pcm_amd import _lib
    X = torch.zeros(4, 3)
    for fn in (pcm_amd.radius_support, pcm_amd.filter_outliers):
        with pytest.raises(_lib.PcmError, match="no CPU fallback"):
            fn(X, 1.0)
    with pytest.raises(ValueError, match="min_neighbors"):
        pcm_amd.filter_outliers(X, 1.0, -1)
    with pytest.raises(ValueError, match="min_days"):
        pcm_amd.filter_outliers(X, 1.0, 1, min_days=0)
    with pytest.raises(ValueError, match="needs groups"):
        pcm_amd.filter_outliers(X, 1.0, 1, min_days=2)
    from pcm_amd import support
    for bad in (0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, "x"):
        with pytest.raises(ValueError, match="radius"):
            support._radius32(bad)
    with pytest.raises(ValueError, match="n_groups must be 1..64"):
        support._groups8(None, 4, 65)


# ---------------------------------------------------------------- the plugin
def stub_fit(X, C0, max_iter, tol_abs):
    f = R.lloyd_fit(np.asarray(X, dtype=np.float32), C0, max_iter=max_iter, tol=tol_abs)
    return f["labels"], f["centers"], f["inertia"], f["n_iter"]


def stub_assign(X, C):
    labels = R.assign(X, C)
    sq = R.sqdist_rows(X, C[labels])
    return labels, sq, float(sq.astype(np.float64).sum())


def ref_support(X, groups, G, radius, min_neighbors, min_days):
    return S.keep_mask(X, radius, min_neighbors, min_days, groups=groups, n_groups=G)


def same_layers(a, b):
    assert len(a) == len(b)
    for (da, pa, ka), (db, pb, kb) in zip(a, b):
        assert ka == kb and pa["name"] == pb["name"] and np.array_equal(da, db, equal_nan=True)
        assert set(pa) == set(pb)
        for key, va in pa.get("properties", {}).items():
            assert np.array_equal(va, pb["properties"][key], equal_nan=True), key


def three_days(m=400, seed=2):
    """Three days of one gentle surface on a shared 20 x 20 raster, each with planted speckle: day g
    gets 5 points far off the surface; day 0 also has a patch nobody else sees."""
    rng = np.random.default_rng(seed)
    clouds = []
    for g in range(3):
        yy, xx = np.divmod(rng.choice(400, m, replace=False), 20)
        z = 0.1 * np.sin(xx / 3.0) + 0.05 * g
        c = np.stack([z, yy.astype(np.float64), xx.astype(np.float64)], axis=1)
        speckle = np.stack([rng.uniform(15, 40, 5), rng.uniform(0, 20, 5), rng.uniform(0, 20, 5)], axis=1)
        clouds.append(np.concatenate([c, speckle]))
    patch = np.stack([np.zeros(9), 40.0 + np.repeat(np.arange(3.0), 3), 40.0 + np.tile(np.arange(3.0), 3)], axis=1)
    clouds[0] = np.concatenate([clouds[0], patch])
    return clouds


def test_plugin_without_denoise_is_unchanged():
    from pcm_amd import plugin
    clouds = three_days()

    def forbidden(*a):
        raise AssertionError("denoise=None must not filter")

    l0, r0 = plugin.kmeans_fuse(clouds, n_clusters=16, max_iter=8, fit=stub_fit)
    l1, r1 = plugin.kmeans_fuse(clouds, n_clusters=16, max_iter=8, fit=stub_fit, denoise=None, support=forbidden)
    same_layers(l0, l1)
    assert set(r0) == set(r1) and "denoise" not in r1
    for key in r0:
        assert np.array_equal(r0[key], r1[key]), key
    a0, s0 = plugin.kmeans_assign(clouds[1:], r0, assign=stub_assign)
    a1, s1 = plugin.kmeans_assign(clouds[1:], r0, assign=stub_assign, denoise=None, support=forbidden)
    same_layers(a0, a1)
    assert set(s0) == set(s1) and "denoise" not in s1
    for key in s0:
        assert np.array_equal(s0[key], s1[key]), key


def test_plugin_fuse_with_denoise():
    from pcm_amd import plugin
    clouds = three_days()
    sizes = [c.shape[0] for c in clouds]
    X = np.concatenate(clouds).astype(np.float32)
    groups = np.repeat(np.arange(3), sizes)
    seen = []

    def spy(X_, groups_, G, radius, min_neighbors, min_days):
        seen.append((X_.copy(), np.asarray(groups_).copy(), G, radius, min_neighbors, min_days))
        return ref_support(X_, groups_, G, radius, min_neighbors, min_days)

    layers, res = plugin.kmeans_fuse(clouds, n_clusters=16, max_iter=8, fit=stub_fit, denoise=(1.5, 2), support=spy)
    assert len(seen) == 1 and np.array_equal(seen[0][0], X) and np.array_equal(seen[0][1], groups)
    assert seen[0][2:] == (3, 1.5, 2, 1)
    den = res["denoise"]
    want = S.keep_mask(X, 1.5, 2)
    assert den["kept"].dtype == bool and np.array_equal(den["kept"], want)
    assert (den["radius"], den["min_neighbors"], den["min_days"]) == (1.5, 2, 1)
    assert den["removed"] == [int((~want[groups == g]).sum()) for g in range(3)] == [5, 5, 5]   # the speckle, not the patch
    assert res["n_points"] == int(want.sum()) and res["labels"].shape == (int(want.sum()),)
    assert np.array_equal(layers[1][0], X[want].astype(np.float64))
    # the same as fusing the pre-filtered clouds
    pre = [c[want[groups == g]] for g, c in enumerate(clouds)]
    l2, r2 = plugin.kmeans_fuse(pre, n_clusters=16, max_iter=8, fit=stub_fit)
    same_layers(layers, l2)
    for key in r2:
        assert np.array_equal(res[key], r2[key]), key
    # min_days = 2 also drops day 0's private patch
    _, res3 = plugin.kmeans_fuse(clouds, n_clusters=16, max_iter=8, fit=stub_fit, denoise=(1.5, 2, 2), support=spy)
    assert seen[-1][2:] == (3, 1.5, 2, 2)
    assert np.array_equal(res3["denoise"]["kept"], S.keep_mask(X, 1.5, 2, 2, groups, 3))
    assert res3["denoise"]["removed"] == [14, 5, 5] and res3["denoise"]["min_days"] == 2


def test_plugin_denoise_feeds_describe_and_height_map_the_kept_rows():
    from pcm_amd import plugin
    clouds = three_days()
    got = {}

    def stats(X_, labels, groups, k, G):
        got["stats"] = (X_.shape[0], labels.shape[0], groups.shape[0], G)
        return np.zeros((G, k, 16), dtype=np.int64)

    def grid(X_, labels, groups, k, G, shape, cell_log2, q):
        got["grid"] = (X_.shape[0], labels.shape[0], groups.shape[0], G)
        return np.zeros((G, 4) + tuple(shape), dtype=np.int64), 0

    _, res = plugin.kmeans_fuse(clouds, n_clusters=8, max_iter=4, fit=stub_fit, denoise=(1.5, 2), support=ref_support,
                                describe=True, stats=stats, height_map=True, grid=grid)
    kept = int(res["denoise"]["kept"].sum())
    assert got["stats"] == (kept, kept, kept, 3) and got["grid"] == (kept, kept, kept, 3)
    assert res["stats"]["sizes"] == res["height_map"]["sizes"] == [c.shape[0] - 5 for c in clouds]


def test_plugin_assign_with_denoise():
    from pcm_amd import plugin
    clouds = three_days()
    _, model = plugin.kmeans_fuse(clouds[:1], n_clusters=16, max_iter=8, fit=stub_fit)
    layers, res = plugin.kmeans_assign(clouds[1:], model, assign=stub_assign, denoise=(1.5, 2), support=ref_support)
    X = np.concatenate(clouds[1:]).astype(np.float32)
    want = S.keep_mask(X, 1.5, 2)
    assert np.array_equal(res["denoise"]["kept"], want) and res["denoise"]["removed"] == [5, 5]
    assert res["n_points"] == int(want.sum()) and np.array_equal(layers[0][0], X[want].astype(np.float64))
    with pytest.raises(ValueError, match="min_neighbors"):
        plugin.kmeans_assign(clouds[1:], model, assign=stub_assign, denoise=(1.5, 2, 2), support=ref_support)


def test_plugin_denoise_errors():
    from pcm_amd import plugin
    tiny = [np.array([[0.0, i, 0.0], [0.0, i, 1.0]]) for i in range(65)]
    with pytest.raises(ValueError, match="at most 64 clouds"):
        plugin.kmeans_fuse(tiny, n_clusters=2, fit=stub_fit, denoise=(1.5, 1, 2), support=ref_support)
    _, res = plugin.kmeans_fuse(tiny, n_clusters=2, max_iter=2, fit=stub_fit, denoise=(1.5, 1), support=ref_support)
    assert res["denoise"]["kept"].all() and len(res["denoise"]["removed"]) == 65      # min_days = 1: any number of clouds
    clouds = three_days()
    for bad in ((1.5,), (0.0, 1), (float("nan"), 1), (1.5, -1), (1.5, 1, 0), 3.0):
        with pytest.raises(ValueError, match="denoise"):
            plugin.kmeans_fuse(clouds, n_clusters=8, fit=stub_fit, denoise=bad, support=ref_support)
    with pytest.raises(ValueError, match="removed every point"):
        plugin.kmeans_fuse(clouds, n_clusters=8, fit=stub_fit, denoise=(1e-3, 1), support=ref_support)

    class Base:
        def run(self, kml_path, **kw):
            return [(c, {"name": f"pair {i} {plugin.CLOUD_LAYER_SUFFIX}"}, "points") for i, c in enumerate(clouds)]

    ex = plugin.HeightMapExtractor(base=Base(), n_clusters=8, max_iter=4, fit=stub_fit, denoise=(1.5, 2),
                                   support=ref_support)
    out = ex.run("x.kml")
    assert len(out) == 5 and ex.last_result["denoise"]["removed"] == [5, 5, 5]
    out = plugin.HeightMapExtractor(base=Base(), n_clusters=8, max_iter=4, fit=stub_fit, denoise=(1.5,),
                                    support=ref_support).run("x.kml")
    assert len(out) == 1 and out[0][1]["name"].startswith("Error:") and "denoise" in out[0][1]["name"]
