"""CPU: the nearest-point reference (tests/nearest_ref.py) -- its cell restatement against its brute
force on two clouds, faces included --, the header and the argument checks of the three entry
points and of the Python layer, and the plugin's ``change=`` paths through the ``nearest=``
stand-in (the product has no CPU fallback; the HIP kernel is checked in tests/test_gpu_nearest.py).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import nearest_ref as N
from oracle import lloyd_ref as R


def same(got, want):
    """Index and distance of ``cells`` / ``brute``: equal, bit for bit."""
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


# ---------------------------------------------------------------- the reference itself
def test_reference_semantics_on_a_hand_case():
    X = np.array([[0, 0, 0], [0, 0, 2], [0, 0, 10], [np.nan, 0, 0]], dtype=np.float32)
    Y = np.array([[0, 0, 1], [0, 0, -1], [0, np.inf, 0], [0, 0, 3], [0, 0, 1]], dtype=np.float32)
    index, sq, skipped, skipped_t, tied = N.brute(X, Y, 1.0)
    assert index.tolist() == [0, 0, -1, -1] and sq.tolist() == [1.0, 1.0, np.inf, np.inf]
    assert (skipped, skipped_t, tied) == (1, 1, 2)                    # rows 0 and 1 have three and three candidates
    index, sq, *_ = N.brute(X, Y, 1.0, gx=[-5, -5, 0, 0], gy=[-5, 0, 0, 7, -5])
    assert index.tolist() == [1, 3, -1, -1]                           # equal groups are no candidates
    assert N.brute(X, Y[:0], 1.0)[0].tolist() == [-1] * 4 and N.brute(X[:0], Y, 1.0)[0].shape == (0,)


@pytest.mark.parametrize("r, s, share", ((0.74, 0, 0.138), (1.48, 1, 0.666)))
def test_cells_equal_brute_force_on_general_floats(r, s, share):
    X, Y = N.general_clouds()
    want = N.brute(X, Y, r)
    got = N.cells(X, Y, r)
    same(got, want)
    assert got[2] == s and abs((want[0] >= 0).mean() - share) < 0.001


@pytest.mark.parametrize("r, share", ((0.75, 0.055), (1.25, 0.236), (2.5, 0.879)))
def test_cells_equal_brute_force_on_the_lattice(r, share):
    X, Y = N.lattice_clouds()
    want = N.brute(X, Y, r)
    same(N.cells(X, Y, r), want)
    assert abs((want[0] >= 0).mean() - share) < 0.001
    assert (want[1] == np.float32(r) * np.float32(r)).any()           # pairs at exactly r: <= is pinned


def test_cells_equal_brute_force_with_groups_on_one_cloud():
    X, _ = N.lattice_clouds()
    days = np.random.default_rng(11).integers(0, 3, 3000)
    want = N.brute(X, X, 1.25, days, days)
    same(N.cells(X, X, 1.25, days, days), want)
    assert abs((want[0] >= 0).mean() - 0.192) < 0.001
    found = want[0] >= 0
    assert (days[want[0][found]] != days[found]).all()
    own = np.arange(3000)
    same(N.cells(X, X, 1.25, own, own), N.brute(X, X, 1.25, own, own))


def test_cells_equal_brute_force_on_ties():
    X, Y = N.tie_clouds()
    want = N.brute(X, Y, 1.5)
    same(N.cells(X, Y, 1.5), want)
    assert ((want[0] >= 0).sum(), want[4], (want[1] == 0).sum()) == (695, 384, 221)
    perm = np.random.default_rng(23).permutation(600)
    same(N.cells(X, Y[perm], 1.5), N.brute(X, Y[perm], 1.5))


@pytest.mark.parametrize("r", (0.5, 1.0, 1.25, 3.0))
def test_cells_equal_brute_force_on_the_faces(r):
    F = N.face_cloud(r)
    perm = np.random.default_rng(31).permutation(F.shape[0])
    own = np.arange(F.shape[0])
    want = N.brute(F, F[perm], r, own, perm)
    got = N.cells(F, F[perm], r, own, perm)
    same(got, want)
    assert got[2] == N.radius_exponent(r) == {0.5: 0, 1.0: 1, 1.25: 1, 3.0: 2}[r]
    assert (want[0] >= 0).all() and F.shape[0] == 102
    assert (want[1] == np.float32(r) * np.float32(r)).sum() == 12 and want[4] > 30


def test_cells_follow_the_box_of_both_clouds():
    # the targets alone would need s = -6; the far query forces the common cells coarser
    Y = (np.random.default_rng(9).random((400, 3)) * 0.05).astype(np.float32)
    X = np.concatenate([Y[:50] + np.float32(0.003), np.float32([[0, 0, 1e6]])])
    s, clo = N.plan(X, Y, 0.01)
    assert N.radius_exponent(0.01) == -6 and s == -1
    same(N.cells(X, Y, 0.01), N.brute(X, Y, 0.01))
    s, clo = N.plan(Y[:0], Y[:0], 0.01)                                # no finite row: the radius alone
    assert s == -6 and not clo.any()


# ---------------------------------------------------------------- the C ABI without a device
@pytest.fixture(scope="module")
def lib():
    from pcm_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.load(require_gpu_runtime=False)


def test_header_declares_the_entry_points_and_constants():
    from pcm_amd import _lib
    src = open(os.path.join(_lib.REPO_DIR, "include", "pcm_kmeans.h")).read()
    for name in ("pcm_nearest_workspace", "pcm_nearest_keys", "pcm_nearest_find"):
        assert re.search(rf"\bint {name}\(", src) and name in _lib.EXPORTS
    for name, value in (("CHUNK", _lib.NEAREST_CHUNK), ("TPB", _lib.NEAREST_TPB),
                        ("INFO_WORDS", _lib.NEAREST_INFO_WORDS)):
        assert int(re.search(rf"#define PCM_NEAREST_{name} (\d+)", src).group(1)) == value
    assert _lib.NEAREST_CHUNK % 64 == 0 and _lib.NEAREST_TPB % 64 == 0 and _lib.NEAREST_INFO_WORDS > 16
    assert int(re.search(r"#define PCM_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 8
    assert os.path.join(_lib.PKG_DIR, "csrc", "pcm_nearest.hip") in _lib.sources()


def test_nearest_argument_errors_without_device(lib):
    from pcm_amd import _lib
    f = ctypes.c_float
    nbytes = ctypes.c_size_t()
    assert lib.pcm_nearest_workspace(-1, ctypes.byref(nbytes)) == -1
    assert "pcm_nearest_workspace" in _lib.last_error()
    assert lib.pcm_nearest_workspace(1 << 31, ctypes.byref(nbytes)) == -1
    assert lib.pcm_nearest_workspace(10, None) == -1
    assert lib.pcm_nearest_workspace(1000, ctypes.byref(nbytes)) == 0 and nbytes.value >= 1000 * 20
    assert lib.pcm_nearest_workspace(0, ctypes.byref(nbytes)) == 0

    one = ctypes.c_void_p(8)          # a non-null pointer that is never followed: the checks come first
    for n, m in ((-1, 5), (5, -1), (1 << 31, 5), (5, 1 << 31)):
        assert lib.pcm_nearest_keys(one, n, one, m, f(1.0), one, one, one, None) == -1
        assert "pcm_nearest_keys" in _lib.last_error() and "n and m must be" in _lib.last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30, 1e-30):   # the last two: the square overflows / is 0
        assert lib.pcm_nearest_keys(one, 5, one, 5, f(bad), one, one, one, None) == -1
        assert "pcm_nearest_keys" in _lib.last_error() and "radius" in _lib.last_error()
    assert lib.pcm_nearest_keys(one, 5, one, 5, f(1.0), one, one, None, None) == -1       # no info block
    assert lib.pcm_nearest_keys(None, 5, one, 5, f(1.0), one, one, one, None) == -1       # no queries
    assert lib.pcm_nearest_keys(one, 5, one, 5, f(1.0), one, None, one, None) == -1       # no target keys
    assert "null" in _lib.last_error()

    def find(n=5, m=5, r=1.0, X=one, groups=None, tgroups=None, index=one, ws=one, ws_bytes=1 << 20):
        return lib.pcm_nearest_find(X, n, one, m, groups, tgroups, f(r), one, one, one, one, index, one, one, ws,
                                    ws_bytes, None)

    for n, m in ((-1, 5), (5, -1), (1 << 31, 5), (5, 1 << 31)):
        assert find(n=n, m=m) == -1
        assert "pcm_nearest_find" in _lib.last_error() and "n and m must be" in _lib.last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30, 1e-30):
        assert find(r=bad) == -1 and "radius" in _lib.last_error()
    assert find(groups=one) == -1 and "go together" in _lib.last_error()
    assert find(tgroups=one) == -1 and "go together" in _lib.last_error()
    assert find(index=None) == -1 and "null" in _lib.last_error()
    assert find(X=None) == -1 and "null" in _lib.last_error()
    assert find(ws=None) == -1 and "workspace" in _lib.last_error()
    assert find(ws_bytes=5 * 20) == -1 and "workspace" in _lib.last_error()
    assert find(n=0) == 0                                                                 # no query: no device call


# ---------------------------------------------------------------- the Python layer
def test_python_validation_without_device():
    torch = pytest.importorskip("torch")
    import pcm_amd
    from pcm_amd import _lib, nearest
    assert pcm_amd.nearest_points is nearest.nearest_points and pcm_amd.Nearest is nearest.Nearest
    assert {"nearest_points", "Nearest"} <= set(pcm_amd.__all__) and "nearest_points(" in pcm_amd.__doc__
    X = torch.zeros(4, 3)
    with pytest.raises(_lib.PcmError, match="no CPU fallback"):
        pcm_amd.nearest_points(X, X, 1.0)
    for bad in (0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, 1e30, 1e-30, "x", None):
        with pytest.raises(ValueError, match="max_dist"):
            nearest._max_dist32(bad)
    assert nearest._max_dist32(0.74) == np.float32(0.74)
    for bad in (torch.zeros(4), torch.zeros(4, dtype=torch.bool), torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="groups must be an integer device tensor"):
            nearest._groups32(bad, 4, "groups")
    near = nearest.Nearest(index=torch.tensor([2, -1], dtype=torch.int32),
                           sqdist=torch.tensor([4.0, float("inf")]), skipped=0, skipped_targets=0, max_dist=3.0,
                           cell_log2=2)
    assert near.found().tolist() == [True, False] and near.distance().tolist() == [2.0, float("inf")]


# ---------------------------------------------------------------- the plugin
def stub_fit(X, C0, max_iter, tol_abs):
    f = R.lloyd_fit(np.asarray(X, dtype=np.float32), C0, max_iter=max_iter, tol=tol_abs)
    return f["labels"], f["centers"], f["inertia"], f["n_iter"]


def stub_assign(X, C):
    labels = R.assign(X, C)
    sq = R.sqdist_rows(X, C[labels])
    return labels, sq, float(sq.astype(np.float64).sum())


def ref_nearest(X, Y, max_dist):
    return N.brute(X, Y, max_dist)[:2]


def two_days(seed=2):
    """An earlier and a later day of one gentle surface on a 20 x 20 raster; the later day is
    shifted by a sub-pixel motion, has a raised patch and five points far off everything."""
    rng = np.random.default_rng(seed)
    yy, xx = np.divmod(np.arange(400), 20)
    early = np.stack([0.1 * np.sin(xx / 3.0), yy.astype(np.float64), xx.astype(np.float64)], axis=1)
    late = early[rng.choice(400, 300, replace=False)] + np.array([0.02, 0.3, -0.2])
    late[:40, 0] += 0.5
    far = np.stack([rng.uniform(15, 40, 5), rng.uniform(0, 20, 5), rng.uniform(0, 20, 5)], axis=1)
    return early, np.concatenate([late, far])


@pytest.fixture(scope="module")
def days():
    from pcm_amd import plugin
    early, late = two_days()
    _, model = plugin.kmeans_fuse([early], n_clusters=16, max_iter=8, fit=stub_fit)
    return early, late, model


def check_change(layers, res, late, ref, r):
    X32, Y32 = late.astype(np.float32), ref.astype(np.float32)
    index, sq, *_ = N.brute(X32, Y32, r)
    found = index >= 0
    assert 0 < found.sum() < found.size                               # NaN where nothing is within max_dist
    want_d = np.where(found, np.sqrt(sq.astype(np.float64)), np.nan)
    want_dz = np.full(found.size, np.nan)
    want_dz[found] = X32[found, 0].astype(np.float64) - Y32[index[found], 0].astype(np.float64)
    props = layers[0][1]["properties"]
    assert props["change"].dtype == np.float64 and props["change_dz"].dtype == np.float64
    assert np.array_equal(props["change"], want_d, equal_nan=True)
    assert np.array_equal(props["change_dz"], want_dz, equal_nan=True)
    assert np.isnan(props["change"][~found]).all() and np.isnan(props["change_dz"][~found]).all()
    ch = res["change"]
    assert set(ch) == {"index", "distance", "dz", "max_dist", "found"}
    assert ch["index"].dtype == np.int32 and np.array_equal(ch["index"], index)
    assert np.array_equal(ch["distance"], want_d, equal_nan=True) and np.array_equal(ch["dz"], want_dz, equal_nan=True)
    assert ch["found"].dtype == bool and np.array_equal(ch["found"], found) and ch["max_dist"] == float(np.float32(r))
    return found


def test_plugin_assign_with_change(days):
    from pcm_amd import plugin
    early, late, model = days
    seen = []

    def spy(X, Y, max_dist):
        seen.append((X.copy(), Y.copy(), max_dist))
        return ref_nearest(X, Y, max_dist)

    layers, res = plugin.kmeans_assign([late], model, assign=stub_assign, change=0.6, change_to=early, nearest=spy)
    assert len(seen) == 1 and seen[0][0].dtype == seen[0][1].dtype == np.float32
    assert np.array_equal(seen[0][0], late.astype(np.float32)) and np.array_equal(seen[0][1], early.astype(np.float32))
    assert seen[0][2] == float(np.float32(0.6))
    found = check_change(layers, res, late, early, 0.6)
    assert not found[-5:].any() and found[40:300].all()               # the far points; the unchanged surface
    # a list of clouds is their concatenation
    l2, r2 = plugin.kmeans_assign([late], model, assign=stub_assign, change=0.6, change_to=[early[:150], early[150:]],
                                  nearest=ref_nearest)
    assert np.array_equal(r2["change"]["index"], res["change"]["index"])
    assert np.array_equal(l2[0][1]["properties"]["change"], layers[0][1]["properties"]["change"], equal_nan=True)


def test_plugin_change_runs_on_the_rows_that_are_labelled(days):
    from pcm_amd import plugin
    import support_ref as S
    early, late, model = days
    layers, res = plugin.kmeans_assign([late], model, assign=stub_assign, denoise=(1.5, 2), change=0.6, change_to=early,
                                       support=lambda X, g, G, r, k, d: S.keep_mask(X, r, k, d), nearest=ref_nearest)
    kept = res["denoise"]["kept"]
    assert 0 < (~kept).sum() and res["change"]["index"].shape == (int(kept.sum()),) == res["labels"].shape
    check_change(layers, res, late[kept], early, 0.6)


def test_plugin_change_takes_the_models_points(days, tmp_path):
    from pcm_amd import plugin
    early, late, model = days
    with pytest.raises(ValueError, match="change_to"):
        plugin.kmeans_assign([late], model, assign=stub_assign, change=0.6, nearest=ref_nearest)
    path = str(tmp_path / "fused.npz")
    plugin.export_fused(path, early, model)
    for m in (path, plugin.load_fused(path), dict(model, points=early)):
        layers, res = plugin.kmeans_assign([late], m, assign=stub_assign, change=0.6, nearest=ref_nearest)
        check_change(layers, res, late, early, 0.6)
    # change_to wins over the model's points
    layers, res = plugin.kmeans_assign([late], path, assign=stub_assign, change=0.6, change_to=early[:100],
                                       nearest=ref_nearest)
    check_change(layers, res, late, early[:100], 0.6)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30, "x"):
        with pytest.raises(ValueError, match="change"):
            plugin.kmeans_assign([late], model, assign=stub_assign, change=bad, change_to=early, nearest=ref_nearest)
    with pytest.raises(ValueError, match="change_to"):
        plugin.kmeans_assign([late], model, assign=stub_assign, change=0.6, change_to=np.zeros((4, 2)),
                             nearest=ref_nearest)
    with pytest.raises(ValueError, match="nearest must return"):
        plugin.kmeans_assign([late], model, assign=stub_assign, change=0.6, change_to=early,
                             nearest=lambda X, Y, r: (np.full(X.shape[0], 400), np.zeros(X.shape[0])))


def test_plugin_without_change_is_unchanged(days):
    from pcm_amd import plugin
    early, late, model = days

    def forbidden(*a):
        raise AssertionError("change=None must not look anything up")

    l0, r0 = plugin.kmeans_assign([late], model, assign=stub_assign, describe=True,
                                  stats=lambda X, lab, g, k, G: np.zeros((G, k, 16), dtype=np.int64))
    l1, r1 = plugin.kmeans_assign([late], model, assign=stub_assign, describe=True,
                                  stats=lambda X, lab, g, k, G: np.zeros((G, k, 16), dtype=np.int64),
                                  change=None, change_to=early, nearest=forbidden)
    assert len(l0) == len(l1) == 2 and set(r0) == set(r1) == {"labels", "distance", "inertia", "n_points", "stats"}
    for (da, pa, ka), (db, pb, kb) in zip(l0, l1):
        assert ka == kb and np.array_equal(da, db) and set(pa) == set(pb)
        assert set(pa["properties"]) == set(pb["properties"])
        for key, va in pa["properties"].items():
            assert np.array_equal(va, pb["properties"][key], equal_nan=True), key
    assert set(l1[0][1]["properties"]) == {"cluster", "residual", "height"}
    for key in ("labels", "distance", "inertia", "n_points"):
        assert np.array_equal(r0[key], r1[key]), key


def test_height_map_extractor_passes_change_on(days):
    from pcm_amd import plugin
    early, late, model = days

    class Base:
        def run(self, kml_path, **kw):
            return [(late, {"name": f"pair 0 {plugin.CLOUD_LAYER_SUFFIX}"}, "points")]

    ex = plugin.HeightMapExtractor(base=Base(), model=model, assign=stub_assign, change=0.6, change_to=early,
                                   nearest=ref_nearest)
    out = ex.run("x.kml")
    assert len(out) == 2
    check_change(out[1:], ex.last_result, late, early, 0.6)
    # without reference points the run comes back as the error layer, naming the argument
    out = plugin.HeightMapExtractor(base=Base(), model=model, assign=stub_assign, change=0.6,
                                    nearest=ref_nearest).run("x.kml")
    assert len(out) == 1 and out[0][1]["name"].startswith("Error:") and "change_to" in out[0][1]["name"]
    plain = plugin.HeightMapExtractor(base=Base(), model=model, assign=stub_assign)
    assert "change" not in plain.run("x.kml")[1][1]["properties"] and "change" not in plain.last_result
