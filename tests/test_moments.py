"""CPU: the local-moments reference (tests/moments_ref.py) -- its cell restatement against its brute
force, the bound on the offsets, the planes --, the header and the argument checks of the three
entry points and of the Python layer, and the plugin's ``change_plane=`` paths through the
``planes=`` stand-in (the product has no CPU fallback; the HIP kernels are checked in
tests/test_gpu_moments.py).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import moments_ref as M
import nearest_ref as N
import support_ref as S
from oracle import lloyd_ref as R


def same(got, want):
    assert got.shape == want.shape and all(int(a) == int(b) for a, b in zip(got.ravel(), want.ravel()))


def check_cells(X, Y, r):
    """``cells == brute`` with the default q, and |dq_a| <= B_a over the pairs the predicate admits."""
    q = M.default_q(X, Y, r)
    want, skipped, skipped_t = M.brute(X, Y, r, q)
    got, s = M.cells(X, Y, r, q)
    same(got, want)
    worst = M.max_offset(X, Y, r, q)
    assert all(int(worst[a]) <= M.bound(r, q[a]) for a in range(3))
    assert all(M.bound(r, v) < 1 << 31 and max(Y.shape[0], 1) * M.bound(r, v) ** 2 <= 1 << 62 for v in q)
    assert max(np.abs(M.fixed(X, q)).max(), np.abs(M.fixed(Y, q)).max()) < 1 << 31
    return want, q, s


# ---------------------------------------------------------------- the reference itself
def test_reference_semantics_on_a_hand_case():
    X = np.array([[0, 0, 0], [0, 0, 2], [np.nan, 0, 0], [0, 0, 10]], dtype=np.float32)
    Y = np.array([[0, 0, 1], [0, 0.5, -0.5], [0, np.inf, 0], [0, 0, 3], [0.25, 0, 1]], dtype=np.float32)
    words, skipped, skipped_t = M.brute(X, Y, 1.0, (2, 2, 2))
    assert (skipped, skipped_t) == (1, 1)
    # row 0: (0,0,1) at exactly r and (0,.5,-.5); (.25,0,1) is beyond r.  dq = (0,0,4), (0,2,-2)
    assert [int(v) for v in words[0]] == [2, 0, 2, 2, 0, 0, 0, 4, -4, 20]
    # row 1: (0,0,1) and (0,0,3) at exactly r: dq = (0,0,-4), (0,0,4)
    assert [int(v) for v in words[1]] == [2, 0, 0, 0, 0, 0, 0, 0, 0, 32]
    assert not any(words[2]) and not any(words[3])                    # a NaN query; a query with no target near
    same(M.cells(X, Y, 1.0, (2, 2, 2))[0], words)
    assert not M.brute(X, Y[:0], 1.0, (2, 2, 2))[0].any() and M.brute(X[:0], Y, 1.0, (2, 2, 2))[0].shape == (0, 10)
    own, *_ = M.brute(X, X, 1.0, (2, 2, 2))                           # one cloud: the row itself counts
    assert [int(w[0]) for w in own] == [1, 1, 0, 1]
    assert M.as_int64(words).dtype == np.int64


@pytest.mark.parametrize("r", (0.75, 1.25, 2.5))
def test_cells_equal_brute_force_on_one_lattice_cloud(r):
    X = S.lattice_cloud()
    want, q, s = check_cells(X, X, r)
    counts = np.array([int(w[0]) for w in want])
    assert np.array_equal(counts, S.brute(X, r)[0].astype(np.int64) + 1)      # support's count and the row itself
    assert s == S.plan(X, r)[0] and (counts > 1).mean() > 0.03


@pytest.mark.parametrize("r", (0.74, 1.48))
def test_cells_equal_brute_force_on_general_floats(r):
    X, Y = N.general_clouds()
    want, q, s = check_cells(X, Y, r)
    found = np.array([int(w[0]) > 0 for w in want])
    assert np.array_equal(found, N.brute(X, Y, r)[0] >= 0) and 0.05 < found.mean() < 0.95


def test_cells_equal_brute_force_on_the_lattice_pair():
    X, Y = N.lattice_clouds()
    want, q, s = check_cells(X, Y, 1.25)
    assert max(q) < M.qcap(2500, 1.25)                                # fixed_q of the box, far below the cap
    assert all(2.0 ** 24 <= v * 2.0 ** e < 2.0 ** 25 for v, e in zip(M.maxabs(X, Y), q))


@pytest.mark.parametrize("r", (0.5, 1.0, 1.25, 3.0))
def test_cells_equal_brute_force_on_the_faces(r):
    F = N.face_cloud(r)
    perm = np.random.default_rng(31).permutation(F.shape[0])
    want, q, s = check_cells(F, F[perm], r)
    assert s == N.radius_exponent(r) and all(int(w[0]) >= 2 for w in want)    # itself and its partner at exactly r


def test_bound_and_default_q():
    from pcm_amd import moments
    for r in (0.5, 1.6, 2.5, 1e-3, 1e4):
        for q in (-126, -3, 0, 7, 18, 40, 62):
            assert M.bound(r, q) == moments.bound(np.float32(r), q)
        for m in (0, 1, 2200, 14_400_000):
            cap = M.qcap(m, r)
            assert cap == moments.q_cap(m, np.float32(r))
            assert max(m, 1) * M.bound(r, cap) ** 2 <= 1 << 62 < max(m, 1) * M.bound(r, cap + 1) ** 2 or cap == 62
    # the 14.4M-point pair cloud at r = 1.6 pixels: 18 bits below a pixel
    assert M.qcap(14_400_000, 1.6) == 18
    X = np.concatenate(M.raster_days()[0])
    assert M.default_q(X, X, 1.6) == (20, 19, 17) == moments.default_q(M.maxabs(X, X), X.shape[0], np.float32(1.6))
    with pytest.raises(ValueError, match="q"):
        moments.check_q((30, 30, 30), M.maxabs(X, X), X.shape[0], np.float32(1.6))
    base = M.clump_cloud()[:2000]
    assert moments.check_q((24, 23, 23), M.maxabs(base, base), 2200, np.float32(2.5)) == (24, 23, 23)
    for bad in ((1, 2), (1, 2, 63), (-127, 0, 0), "abc", 5, (1.5, "x", 2)):
        with pytest.raises(ValueError, match="q must be three integers"):
            moments.check_q(bad, [1.0, 1.0, 1.0], 10, np.float32(1.0))
    with pytest.raises(ValueError, match="reaches 2\\^31"):
        moments.check_q((10, 10, 22), [1.0, 1.0, 600.0], 10, np.float32(1.0))


def test_planes_of_the_reference():
    X = S.lattice_cloud()
    q = M.default_q(X, X, 2.5)
    words, *_ = M.brute(X[:400], X, 2.5, q)
    P = M.planes(words, q, 3)
    c = np.array([int(w[0]) for w in words])
    assert np.array_equal(np.isnan(P["roughness"]), c < 3) and 200 < (c >= 3).sum() < 400
    ok = c >= 3
    for i in np.flatnonzero(ok)[:50]:                                 # against the float64 covariance of the neighbourhood
        near = N.sqdist_block(X[i:i + 1], X)[0] <= np.float32(2.5) ** 2
        d = X[near].astype(np.float64) - X[i].astype(np.float64)
        assert np.allclose(P["cov"][i], np.cov(d.T, bias=True), atol=1e-12) and np.allclose(P["mu"][i], d.mean(0), atol=1e-12)
    nrm = P["normal"][ok]
    assert np.allclose((nrm * nrm).sum(1), 1.0) and (nrm[:, 0] >= 0).all()
    assert np.allclose(P["distance"][ok], -(nrm * P["mu"][ok]).sum(1))
    assert (P["planarity"][ok] >= 0).all() and (P["planarity"][ok] <= 1 + 1e-12).all()
    assert np.isnan(M.planes(words, q, 5)["roughness"]).sum() == (c < 5).sum() > (c < 3).sum()


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
    for name in ("pcm_moments_workspace", "pcm_moments_scan", "pcm_moments_planes"):
        assert re.search(rf"\bint {name}\(", src) and name in _lib.EXPORTS
    for name, value in (("CHUNK", _lib.MOMENTS_CHUNK), ("TPB", _lib.MOMENTS_TPB), ("WORDS", _lib.MOMENTS_WORDS)):
        assert int(re.search(rf"#define PCM_MOMENTS_{name} (\d+)", src).group(1)) == value
    assert _lib.MOMENTS_CHUNK % 64 == 0 and _lib.MOMENTS_TPB % 64 == 0 and _lib.MOMENTS_WORDS == M.WORDS == 10
    assert int(re.search(r"#define PCM_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 8
    assert os.path.join(_lib.PKG_DIR, "csrc", "pcm_moments.hip") in _lib.sources()
    # four waves with a float and an int record per staged row: 16 KB of LDS per block
    assert (_lib.MOMENTS_TPB // 64) * _lib.MOMENTS_CHUNK * 32 == 16384


def test_moments_argument_errors_without_device(lib):
    from pcm_amd import _lib
    f = ctypes.c_float
    nbytes = ctypes.c_size_t()
    assert lib.pcm_moments_workspace(-1, ctypes.byref(nbytes)) == -1
    assert "pcm_moments_workspace" in _lib.last_error()
    assert lib.pcm_moments_workspace(1 << 31, ctypes.byref(nbytes)) == -1
    assert lib.pcm_moments_workspace(10, None) == -1
    assert lib.pcm_moments_workspace(1000, ctypes.byref(nbytes)) == 0 and nbytes.value >= 1000 * 24
    assert lib.pcm_moments_workspace(0, ctypes.byref(nbytes)) == 0

    one = ctypes.c_void_p(8)          # a non-null pointer that is never followed: the checks come first
    q3 = lambda *v: (ctypes.c_int32 * 3)(*v)   # noqa: E731

    def scan(n=5, m=5, r=1.0, X=one, Y=one, q=q3(10, 10, 10), words=one, info=one, ws=one, ws_bytes=1 << 20, perm=one):
        return lib.pcm_moments_scan(X, n, Y, m, f(r), q, one, perm, one, one, words, info, ws, ws_bytes, None)

    for n, m in ((-1, 5), (5, -1), (1 << 31, 5), (5, 1 << 31)):
        assert scan(n=n, m=m) == -1
        assert "pcm_moments_scan" in _lib.last_error() and "n and m must be" in _lib.last_error()
    assert scan(n=-1, Y=None) == -1 and scan(n=1 << 31, Y=None) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30, 1e-30):   # the last two: the square overflows / is 0
        assert scan(r=bad) == -1 and "pcm_moments_scan" in _lib.last_error() and "radius" in _lib.last_error()
    for bad in (q3(63, 0, 0), q3(0, -127, 0), q3(0, 0, 1000), None):
        assert scan(q=bad) == -1 and "pcm_moments_scan: q" in _lib.last_error()
    assert scan(q=q3(62, -126, 0), words=None) == -1 and "words is null" in _lib.last_error()   # the ends of q's range pass
    assert scan(X=None) == -1 and "null" in _lib.last_error()
    assert scan(info=None) == -1 and "null" in _lib.last_error()
    assert scan(perm=None, Y=None) == -1 and "null" in _lib.last_error()
    assert scan(ws=None) == -1 and "workspace" in _lib.last_error()
    assert scan(ws_bytes=5 * 24) == -1 and "workspace" in _lib.last_error()
    assert scan(Y=None, m=0, n=50, ws_bytes=5 * 24) == -1 and "workspace" in _lib.last_error()   # Y null: n targets
    assert scan(n=0) == 0 and scan(n=0, Y=None) == 0                                            # no query: no device call

    def planes(n=5, q=q3(10, 10, 10), min_count=3, words=one, normal=one, rough=one):
        return lib.pcm_moments_planes(words, n, q, min_count, normal, one, rough, one, None)

    for n in (-1, 1 << 31):
        assert planes(n=n) == -1 and "pcm_moments_planes" in _lib.last_error()
    for bad in (q3(63, 0, 0), q3(0, -127, 0), None):
        assert planes(q=bad) == -1 and "pcm_moments_planes: q" in _lib.last_error()
    assert planes(min_count=-1) == -1 and "min_count" in _lib.last_error()
    assert planes(words=None) == -1 and "null" in _lib.last_error()
    assert planes(normal=None) == -1 and planes(rough=None) == -1 and "pcm_moments_planes" in _lib.last_error()
    assert planes(n=0) == 0                                                                     # no row: no device call


# ---------------------------------------------------------------- the Python layer
def test_python_validation_without_device():
    torch = pytest.importorskip("torch")
    import pcm_amd
    from pcm_amd import _lib, moments
    assert pcm_amd.local_moments is moments.local_moments and pcm_amd.point_normals is moments.point_normals
    assert pcm_amd.LocalMoments is moments.LocalMoments and pcm_amd.PointNormals is moments.PointNormals
    assert {"local_moments", "point_normals", "LocalMoments", "PointNormals"} <= set(pcm_amd.__all__)
    assert "local_moments(" in pcm_amd.__doc__ and "point_normals(" in pcm_amd.__doc__
    X = torch.zeros(4, 3)
    with pytest.raises(_lib.PcmError, match="no CPU fallback"):
        pcm_amd.local_moments(X, 1.0)
    with pytest.raises(_lib.PcmError, match="no CPU fallback"):
        pcm_amd.point_normals(X, 1.0)
    for bad in (0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, 1e30, 1e-30, "x", None):
        with pytest.raises(ValueError, match="radius"):
            moments._radius32(bad)
    assert moments._radius32(1.6) == np.float32(1.6)
    for bad in (-1, 2.5, True, None, "3"):
        with pytest.raises(ValueError, match="min_count"):
            pcm_amd.point_normals(X, 1.0, min_count=bad)
    # the float64 views of the words, on a hand-made row: two targets at dq = (0, 0, -4) and (0, 0, 4), q = 2
    lm = moments.LocalMoments(words=torch.tensor([[2, 0, 0, 0, 0, 0, 0, 0, 0, 32], [0] * 10]), q=(2, 2, 2), radius=1.0,
                              skipped=0, skipped_targets=0, cell_log2=1)
    assert lm.counts().tolist() == [2, 0] and lm.offsets()[0].tolist() == [0.0, 0.0, 0.0]
    cov = lm.covariances()
    assert cov.dtype == torch.float64 and cov.shape == (2, 3, 3) and cov[0, 2, 2] == 1.0 and cov[0].sum() == 1.0
    assert torch.isnan(cov[1]).all() and torch.isnan(lm.offsets()[1]).all()
    with pytest.raises(ValueError, match="LocalMoments of this call"):
        pcm_amd.point_normals(torch.zeros(3, 3), 1.0, moments=lm)
    with pytest.raises(ValueError, match="radius or q differs"):
        pcm_amd.point_normals(torch.zeros(2, 3), 2.0, moments=lm)


# ---------------------------------------------------------------- the plugin
def stub_fit(X, C0, max_iter, tol_abs):
    f = R.lloyd_fit(np.asarray(X, dtype=np.float32), C0, max_iter=max_iter, tol=tol_abs)
    return f["labels"], f["centers"], f["inertia"], f["n_iter"]


def stub_assign(X, C):
    labels = R.assign(X, C)
    sq = R.sqdist_rows(X, C[labels])
    return labels, sq, float(sq.astype(np.float64).sum())


def ref_planes(X, Y, radius):
    q = M.default_q(X, Y, radius)
    words, *_ = M.brute(X, Y, radius, q)
    P = M.planes(words, q, 3)
    return P["distance"].astype(np.float32), P["normal"].astype(np.float32), np.array([int(w[0]) for w in words])


def two_days(seed=2):
    """An earlier day of one sloped surface on a 20 x 20 raster and a later one lifted by 0.5 along z,
    with five points far off everything."""
    rng = np.random.default_rng(seed)
    yy, xx = np.divmod(np.arange(400), 20)
    early = np.stack([0.3 * xx + 0.1 * yy, yy.astype(np.float64), xx.astype(np.float64)], axis=1)
    late = early[rng.choice(400, 300, replace=False)] + np.array([0.5, 0.3, -0.2])
    far = np.stack([rng.uniform(25, 40, 5), rng.uniform(0, 20, 5), rng.uniform(0, 20, 5)], axis=1)
    return early, np.concatenate([late, far])


@pytest.fixture(scope="module")
def days():
    from pcm_amd import plugin
    early, late = two_days()
    _, model = plugin.kmeans_fuse([early], n_clusters=16, max_iter=8, fit=stub_fit)
    return early, late, model


def check_plane(layers, res, late, ref, r):
    dist, normal, count = ref_planes(late.astype(np.float32), ref.astype(np.float32), float(np.float32(r)))
    few = count < 3
    assert 0 < few.sum() < few.size
    props = layers[0][1]["properties"]
    assert props["change_normal"].dtype == np.float64 and props["change_normal_z"].dtype == np.float64
    assert np.array_equal(props["change_normal"], np.where(few, np.nan, dist.astype(np.float64)), equal_nan=True)
    assert np.array_equal(props["change_normal_z"], np.where(few, np.nan, normal[:, 0].astype(np.float64)), equal_nan=True)
    cp = res["change_plane"]
    assert set(cp) == {"distance", "normal", "count", "radius"} and cp["radius"] == float(np.float32(r))
    assert np.array_equal(cp["distance"], props["change_normal"], equal_nan=True) and cp["normal"].shape == (few.size, 3)
    assert cp["count"].dtype == np.int64 and np.array_equal(cp["count"], count)
    return few


def test_plugin_assign_with_change_plane(days):
    from pcm_amd import plugin
    early, late, model = days
    seen = []

    def spy(X, Y, radius):
        seen.append((X.copy(), Y.copy(), radius))
        return ref_planes(X, Y, radius)

    layers, res = plugin.kmeans_assign([late], model, assign=stub_assign, change_plane=1.6, change_to=early, planes=spy)
    assert len(seen) == 1 and seen[0][0].dtype == seen[0][1].dtype == np.float32
    assert np.array_equal(seen[0][0], late.astype(np.float32)) and np.array_equal(seen[0][1], early.astype(np.float32))
    assert seen[0][2] == float(np.float32(1.6))
    few = check_plane(layers, res, late, early, 1.6)
    assert few[-5:].all() and "change" not in res and "change" not in layers[0][1]["properties"]
    # the later day is the plane z = 0.1 y + 0.3 x moved by (0.5, 0.3, -0.2): its distance to that plane
    d = layers[0][1]["properties"]["change_normal"][~few]
    assert np.allclose(d, (0.5 - 0.1 * 0.3 + 0.3 * 0.2) / np.sqrt(1 + 0.01 + 0.09), atol=1e-5)
    # together with change=, and a list of clouds is their concatenation
    l2, r2 = plugin.kmeans_assign([late], model, assign=stub_assign, change=0.9, change_plane=1.6,
                                  change_to=[early[:150], early[150:]], planes=ref_planes,
                                  nearest=lambda X, Y, r: N.brute(X, Y, r)[:2])
    assert {"change", "change_dz", "change_normal", "change_normal_z"} <= set(l2[0][1]["properties"])
    assert np.array_equal(r2["change_plane"]["distance"], res["change_plane"]["distance"], equal_nan=True)
    assert "change" in r2


def test_plugin_change_plane_runs_on_the_rows_that_are_labelled(days):
    from pcm_amd import plugin
    early, late, model = days
    layers, res = plugin.kmeans_assign([late], model, assign=stub_assign, denoise=(1.5, 2), change_plane=1.6,
                                       change_to=early, support=lambda X, g, G, r, k, d: S.keep_mask(X, r, k, d),
                                       planes=ref_planes)
    kept = res["denoise"]["kept"]
    assert 0 < (~kept).sum() and res["change_plane"]["count"].shape == (int(kept.sum()),) == res["labels"].shape


def test_plugin_change_plane_needs_reference_points(days, tmp_path):
    from pcm_amd import plugin
    early, late, model = days
    with pytest.raises(ValueError, match="change_plane= needs reference points"):
        plugin.kmeans_assign([late], model, assign=stub_assign, change_plane=1.6, planes=ref_planes)
    path = str(tmp_path / "fused.npz")
    plugin.export_fused(path, early, model)
    for m in (path, dict(model, points=early)):
        layers, res = plugin.kmeans_assign([late], m, assign=stub_assign, change_plane=1.6, planes=ref_planes)
        check_plane(layers, res, late, early, 1.6)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30, "x"):
        with pytest.raises(ValueError, match="change_plane must be None or a radius"):
            plugin.kmeans_assign([late], model, assign=stub_assign, change_plane=bad, change_to=early, planes=ref_planes)
    with pytest.raises(ValueError, match="planes must return"):
        plugin.kmeans_assign([late], model, assign=stub_assign, change_plane=1.6, change_to=early,
                             planes=lambda X, Y, r: (np.zeros(3), np.zeros((3, 3)), np.zeros(3)))


def test_plugin_without_change_plane_is_unchanged(days):
    from pcm_amd import plugin
    early, late, model = days

    def forbidden(*a):
        raise AssertionError("change_plane=None must not solve anything")

    l0, r0 = plugin.kmeans_assign([late], model, assign=stub_assign)
    l1, r1 = plugin.kmeans_assign([late], model, assign=stub_assign, change_plane=None, change_to=early, planes=forbidden)
    assert len(l0) == len(l1) == 1 and set(r0) == set(r1) == {"labels", "distance", "inertia", "n_points"}
    assert set(l1[0][1]["properties"]) == {"cluster", "residual", "height"}
    for key, va in l0[0][1]["properties"].items():
        assert np.array_equal(va, l1[0][1]["properties"][key], equal_nan=True), key
    for key in r0:
        assert np.array_equal(r0[key], r1[key]), key


def test_height_map_extractor_passes_change_plane_on(days):
    from pcm_amd import plugin
    early, late, model = days

    class Base:
        def run(self, kml_path, **kw):
            return [(late, {"name": f"pair 0 {plugin.CLOUD_LAYER_SUFFIX}"}, "points")]

    ex = plugin.HeightMapExtractor(base=Base(), model=model, assign=stub_assign, change_plane=1.6, change_to=early,
                                   planes=ref_planes)
    out = ex.run("x.kml")
    assert len(out) == 2
    check_plane(out[1:], ex.last_result, late, early, 1.6)
    out = plugin.HeightMapExtractor(base=Base(), model=model, assign=stub_assign, change_plane=1.6,
                                    planes=ref_planes).run("x.kml")
    assert len(out) == 1 and out[0][1]["name"].startswith("Error:") and "change_plane" in out[0][1]["name"]
    plain = plugin.HeightMapExtractor(base=Base(), model=model, assign=stub_assign)
    assert "change_normal" not in plain.run("x.kml")[1][1]["properties"] and "change_plane" not in plain.last_result
