"""CPU: ``pcm_cluster_stats``' argument checks, the ``ClusterStats`` accessors and
``surface_elements`` on words from the NumPy reference encoder (tests/stats_ref.py),
and the plugin's ``describe=True`` outputs through the ``stats=`` stand-in (the
product has no CPU fallback; the HIP kernel is checked in tests/test_gpu_stats.py).
"""
import ctypes
import os

import numpy as np
import pytest

import stats_ref as SR
from oracle import lloyd_ref as R


def blobs(n, d, seed, nb=12, sd=0.8):
    rng = np.random.default_rng(seed)
    centers = rng.random((nb, d)) * 10 - 3          # mixed signs
    return (centers[rng.integers(0, nb, n)] + rng.normal(0, sd, (n, d))).astype(np.float32)


def dequantised(X, q):
    return R.to_fixed(X, q).astype(np.float64) * np.ldexp(1.0, -q.astype(np.int64))[None, :]


# ---------------------------------------------------------------- ABI
def test_cluster_stats_argument_errors_without_device():
    """Every argument check runs before any device call; n = 0 makes none."""
    from pcm_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    lib = _lib.load(require_gpu_runtime=False)
    one = ctypes.c_void_p(256)      # a non-null address that is never dereferenced
    q = (ctypes.c_int32 * 4)(0, 0, 0, 0)

    def call(X=one, dtype=0, n=10, d=3, labels=one, groups=None, G=1, k=4, qq=q, out=one):
        return lib.pcm_cluster_stats(X, dtype, n, d, labels, groups, G, k, qq, out, None)

    for kw, word in ((dict(d=0), "d must be"), (dict(d=5), "d must be"), (dict(dtype=2), "dtype"), (dict(dtype=7), "dtype"),
                     (dict(n=-1), "n must be"), (dict(n=1 << 31), "2^31"), (dict(k=0), "k must be"),
                     (dict(G=0), "n_groups"), (dict(G=257), "n_groups"), (dict(out=None), "null"),
                     (dict(labels=None), "null"), (dict(X=None), "null"), (dict(qq=None), "null")):
        assert call(**kw) == -1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert call(n=(1 << 31) - 1, d=7) == -1
    assert call(n=0) == 0
    assert call(n=0, X=None, labels=None, qq=None, out=None) == 0
    assert call(n=0, G=256, k=1 << 20) == 0
    assert _lib.stats_words(3) == 16 and [_lib.stats_words(d) for d in (1, 2, 4)] == [4, 9, 25]


def test_public_names():
    import pcm_amd
    for name in ("cluster_stats", "ClusterStats", "surface_elements"):
        assert name in pcm_amd.__all__ and getattr(pcm_amd, name) is not None
    from pcm_amd import _lib
    assert "pcm_cluster_stats" in _lib.EXPORTS
    assert any(u.endswith("pcm_stats.hip") for u in _lib.UNITS)
    with pytest.raises(_lib.PcmError):
        import torch
        pcm_amd.cluster_stats(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), 2)      # host tensor


# ---------------------------------------------------------------- accessors
@pytest.fixture(scope="module")
def small():
    """3000 points, d = 3, K = 7, G = 3: small enough for Python-int sums."""
    X = blobs(3000, 3, 5)
    C = X[R.init_indices(3000, 7)]
    labels = R.assign(X, C)
    groups = np.random.default_rng(1).integers(0, 3, 3000)
    q = R.fixed_q(X)
    words, skipped = SR.encode(X, labels, 7, q, groups, 3)
    assert skipped == 0
    return X, C, labels, groups, q, words


def test_encoder_matches_python_int_sums(small):
    X, C, labels, groups, q, words = small
    c0, s0, m0 = SR.direct(X, labels, 7, q, groups, 3)
    c1, s1, m1 = SR.decode(words, 3)
    assert (c0 == c1).all() and (s0 == s1).all() and (m0 == m1).all()
    assert (words.view(np.int64)[..., 5::2] < 0).any()      # mixed signs: negative hi-limb sums occur


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_exact_accessors(d):
    from pcm_amd.stats import ClusterStats
    n, k, G = 2000, 5, 2
    X = blobs(n, d, 40 + d)
    labels = R.assign(X, X[R.init_indices(n, k)])
    groups = np.random.default_rng(d).integers(0, G, n)
    q = R.fixed_q(X)
    words, _ = SR.encode(X, labels, k, q, groups, G)
    st = ClusterStats(words, q, d)
    c0, s0, m0 = SR.direct(X, labels, k, q, groups, G)
    assert st.counts().dtype == np.int64 and st.counts().shape == (G, k) and (st.counts() == c0).all()
    assert st.sums().dtype == np.int64 and st.sums().shape == (G, k, d) and (st.sums() == s0).all()
    M = st.moments()
    assert M.shape == (G, k, d, d) and M.dtype == object and (M == m0).all()
    assert all(type(v) is int for v in M.ravel())
    assert (M == np.swapaxes(M, 2, 3)).all()
    # merged: the one-group statistics of the same rows
    w1, _ = SR.encode(X, labels, k, q)
    mg = st.merged()
    assert mg.n_groups == 1 and np.array_equal(mg.numpy().view(np.uint64), w1)
    # __add__: two halves of the rows
    h = n // 2
    wa, _ = SR.encode(X[:h], labels[:h], k, q, groups[:h], G)
    wb, _ = SR.encode(X[h:], labels[h:], k, q, groups[h:], G)
    both = ClusterStats(wa, q, d) + ClusterStats(wb, q, d)
    assert np.array_equal(both.numpy().view(np.uint64), words)
    with pytest.raises(ValueError):
        ClusterStats(wa, q, d) + ClusterStats(wb, q + 1, d)
    with pytest.raises(ValueError):
        ClusterStats(wa, q, d) + mg
    with pytest.raises(ValueError):
        ClusterStats(wa[..., :-1], q, d)


def test_means_are_the_engine_centre_update(small):
    from pcm_amd.stats import ClusterStats
    X, C, labels, groups, q, words = small
    st = ClusterStats(words, q, 3).merged()
    counts, sums = st.counts()[0], st.sums()[0]
    assert (counts > 0).all()
    want = R.average(sums, counts, q, C)
    got = st.means()[0].astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # an empty (group, cluster) is NaN in every derived accessor
    w2 = words.copy()
    w2[1, 3] = 0
    e = ClusterStats(w2, q, 3)
    assert np.isnan(e.means()[1, 3]).all() and np.isnan(e.covariances()[1, 3]).all()
    assert np.isfinite(e.means()[0]).all()
    off = e.offsets(C)
    assert off.shape == (3, 7, 3) and np.array_equal(off[0], e.means()[0] - C.astype(np.float64))


def test_covariances_against_numpy():
    """n = 50 000, K = 16, G = 3 against np.cov(bias=True) of the dequantised
    points: |delta| <= 1e-9 sqrt(var_a var_b) (NumPy's own two-pass error is about
    n 2^-53 = 6e-12 here, so the margin does not hide a wrong limb)."""
    from pcm_amd.stats import ClusterStats
    n, k, G = 50_000, 16, 3
    X = blobs(n, 3, 9)
    labels = R.assign(X, X[R.init_indices(n, k)])
    groups = np.random.default_rng(3).integers(0, G, n)
    q = R.fixed_q(X)
    words, _ = SR.encode(X, labels, k, q, groups, G)
    cov = ClusterStats(words, q, 3).covariances()
    Xd = dequantised(X, q)
    worst = 0.0
    for g in range(G):
        for j in range(k):
            P = Xd[(groups == g) & (labels == j)]
            assert P.shape[0] > 3
            ref = np.cov(P.T, bias=True)
            scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
            worst = max(worst, float(np.max(np.abs(cov[g, j] - ref) / scale)))
    print(f"worst scaled covariance error {worst:.3e}")
    assert worst <= 1e-9


# ---------------------------------------------------------------- surface elements
def test_surface_elements_on_tilted_planes():
    from pcm_amd.stats import ClusterStats, surface_elements
    rng = np.random.default_rng(2)
    normals = np.array([[1.0, 0.0, 0.0], [0.8, 0.6, 0.0], [0.6, -0.48, 0.64], [0.0, 1.0, 0.0], [0.1, -0.7, 0.7]])
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    pts, lab = [], []
    for j, nv in enumerate(normals):
        u = np.linalg.svd(nv[None])[2][1:]                        # two in-plane axes
        m = 400 + 50 * j
        p = rng.uniform(-20, 20, (m, 2)) @ u + rng.normal(0, 0.05, (m, 1)) * nv + rng.uniform(-50, 50, 3)
        pts.append(p)
        lab += [j] * m
    pts.append(np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.5]]))        # cluster 5: two points
    lab += [5, 5]
    pts.append(np.array([[-7.0, 8.0, 9.0]]))                        # cluster 6: one point
    lab += [6]
    X = np.concatenate(pts).astype(np.float32)
    lab = np.asarray(lab, np.int32)
    groups = rng.integers(0, 2, X.shape[0])                         # surface elements merge the groups
    q = R.fixed_q(X)
    words, _ = SR.encode(X, lab, 8, q, groups, 2)                   # cluster 7: empty
    st = ClusterStats(words, q, 3)
    se = surface_elements(st)
    Xd = dequantised(X, q)
    for j in range(5):
        P = Xd[lab == j]
        Pc = P - P.mean(0)
        sv = np.linalg.svd(Pc, full_matrices=False)
        nref = sv[2][2] if sv[2][2][0] >= 0 else -sv[2][2]
        assert se.normal[j, 0] >= 0
        assert abs(np.linalg.norm(se.normal[j]) - 1) < 1e-12
        assert np.linalg.norm(se.normal[j] - nref) < 1e-6, (j, se.normal[j], nref)
        lam = sv[1][::-1] ** 2 / P.shape[0]                         # ascending eigenvalues of the covariance
        assert se.roughness[j] == pytest.approx(np.sqrt(lam[0]), rel=1e-7)
        assert se.planarity[j] == pytest.approx((lam[1] - lam[0]) / lam[2], rel=1e-7)
        assert se.rms[j] == pytest.approx(np.sqrt(lam.sum()), rel=1e-9)
        assert 0.03 < se.roughness[j] < 0.07 and se.planarity[j] > 0.3
    # the sign rule where the normal lies in the z = 0 plane: first non-zero component positive
    assert abs(se.normal[3, 0]) < 1e-2
    for j in (5, 6, 7):                                             # below min_count = 3: all NaN
        assert np.isnan(se.normal[j]).all() and np.isnan(se.roughness[j]) and np.isnan(se.planarity[j]) \
            and np.isnan(se.rms[j])
    assert list(se.count) == [400, 450, 500, 550, 600, 2, 1, 0]
    one = surface_elements(st, min_count=1)
    assert one.roughness[6] == 0.0 and one.rms[6] == 0.0 and one.planarity[6] == 0.0        # a single point
    assert np.isfinite(one.normal[6]).all() and one.roughness[5] == pytest.approx(0.0, abs=1e-6)
    assert np.isnan(one.roughness[7])
    with pytest.raises(ValueError):
        surface_elements(ClusterStats(SR.encode(X[:, :2], lab, 8, q[:2])[0], q[:2], 2))


# ---------------------------------------------------------------- plugin
def oracle_fit_plugin(X, C0, max_iter, tol_abs):
    r = R.lloyd_fit(X, C0, max_iter=max_iter, tol=tol_abs)
    return r["labels"], r["centers"], r["inertia"], r["n_iter"]


def oracle_assign(X, C):
    X, C = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(C, np.float32)
    labels = R.assign(X, C)
    sq = R.sqdist_rows(X, C[labels])
    return labels, sq, R.inertia_exact(sq, R.inertia_scale(R.fixed_q(np.vstack([X, C]))))


def oracle_stats(X, labels, groups, k, G):
    X = np.ascontiguousarray(X, np.float32)
    return SR.encode(X, labels, k, R.fixed_q(X), groups, G)[0]


def three_days():
    """Three clouds over a 60 x 80 relief; the third covers only the left half and
    sits 0.5 higher, so the right-hand elements are seen on two days only."""
    rng = np.random.default_rng(4)
    out = []
    for day in range(3):
        yy, xx = np.mgrid[0:60, 0:80]
        keep = rng.random(yy.shape) > 0.2
        if day == 2:
            keep &= xx < 40
        z = 6 * np.sin(xx / 19.0) + 4 * np.cos(yy / 13.0) + rng.normal(0, 0.2, yy.shape) + (0.5 if day == 2 else 0.0)
        out.append(np.stack([z[keep], yy[keep].astype(np.float64), xx[keep].astype(np.float64)], axis=1))
    return out


def test_kmeans_fuse_describe():
    import pcm_amd
    clouds = three_days()
    k = 12
    base_layers, base = pcm_amd.kmeans_fuse(clouds + [np.zeros((0, 3))], n_clusters=k, fit=oracle_fit_plugin)
    layers, res = pcm_amd.kmeans_fuse(clouds + [np.zeros((0, 3))], n_clusters=k, fit=oracle_fit_plugin, describe=True,
                                      stats=oracle_stats)
    # default output unchanged: same layers, and the same properties and keys apart from the new ones
    assert set(base) == {"labels", "centers", "inertia", "n_iter", "n_points"}
    assert set(base_layers[0][1]["properties"]) == {"height", "count"}
    assert set(res) == set(base) | {"stats"}
    assert [l[1]["name"] for l in layers] == [l[1]["name"] for l in base_layers]
    np.testing.assert_array_equal(res["labels"], base["labels"])
    props = layers[0][1]["properties"]
    assert set(props) == {"height", "count", "roughness", "normal_z", "days_seen", "height_spread"}
    np.testing.assert_array_equal(props["count"], base_layers[0][1]["properties"]["count"])
    assert set(layers[1][1]["properties"]) == set(base_layers[1][1]["properties"])
    # against direct NumPy on the (dequantised) clouds
    X = np.concatenate(clouds).astype(np.float32)
    q = R.fixed_q(X)
    Xd = dequantised(X, q)
    sizes = [c.shape[0] for c in clouds]
    groups = np.repeat(np.arange(3), sizes)
    labels = res["labels"]
    assert res["stats"]["sizes"] == sizes and res["stats"]["q"] == list(q)
    assert res["stats"]["words"].shape == (3, k, 16) and res["stats"]["words"].dtype == np.int64
    np.testing.assert_array_equal(res["stats"]["words"].view(np.uint64), SR.encode(X, labels, k, q, groups, 3)[0])
    seen_two = 0
    for j in range(k):
        P = Xd[labels == j]
        lam, vec = np.linalg.eigh(np.cov(P.T, bias=True))
        assert props["roughness"][j] == pytest.approx(np.sqrt(lam[0]), rel=1e-7)
        assert props["normal_z"][j] == pytest.approx(abs(vec[0, 0]), abs=1e-7) and props["normal_z"][j] >= 0
        days = [g for g in range(3) if np.any((labels == j) & (groups == g))]
        assert props["days_seen"][j] == len(days)
        mz = [Xd[(labels == j) & (groups == g), 0].mean() for g in days]
        want = max(mz) - min(mz) if len(days) >= 2 else 0.0
        assert props["height_spread"][j] == pytest.approx(want, rel=1e-9, abs=1e-12)
        seen_two += len(days) == 2
    assert seen_two > 0 and props["days_seen"].max() == 3          # day 3 misses the right-hand elements
    # an element the raised third day saw has a larger spread than the noise of the means
    assert props["height_spread"][props["days_seen"] == 3].min() > 0.2
    # one cloud: nothing to spread
    l1, _ = pcm_amd.kmeans_fuse(clouds[:1], n_clusters=k, fit=oracle_fit_plugin, describe=True, stats=oracle_stats)
    assert (l1[0][1]["properties"]["height_spread"] == 0).all() and (l1[0][1]["properties"]["days_seen"] == 1).all()


def test_kmeans_fuse_describe_takes_256_clouds_at_most():
    import pcm_amd
    rng = np.random.default_rng(0)
    clouds = [rng.random((2, 3)) for _ in range(257)]
    with pytest.raises(ValueError, match="256"):
        pcm_amd.kmeans_fuse(clouds, n_clusters=4, fit=oracle_fit_plugin, describe=True, stats=oracle_stats)
    layers, res = pcm_amd.kmeans_fuse(clouds[:256], n_clusters=4, fit=oracle_fit_plugin, describe=True,
                                      stats=oracle_stats)
    assert res["stats"]["words"].shape == (256, 4, 16) and res["stats"]["words"][..., 0].sum() == 512
    pcm_amd.kmeans_fuse(clouds, n_clusters=4, fit=oracle_fit_plugin)           # without describe: no limit


def test_kmeans_assign_describe():
    import pcm_amd
    clouds = three_days()
    k = 12
    _, model = pcm_amd.kmeans_fuse(clouds[:2], n_clusters=k, fit=oracle_fit_plugin)
    base_layers, base = pcm_amd.kmeans_assign(clouds[2:], model, assign=oracle_assign)
    layers, res = pcm_amd.kmeans_assign(clouds[2:], model, assign=oracle_assign, describe=True, stats=oracle_stats)
    assert len(base_layers) == 1 and set(base) == {"labels", "distance", "inertia", "n_points"}
    assert len(layers) == 2 and set(res) == set(base) | {"stats"}
    np.testing.assert_array_equal(layers[0][0], base_layers[0][0])
    assert set(layers[0][1]["properties"]) == set(base_layers[0][1]["properties"])
    data, params, kind = layers[1]
    assert kind == "points" and params["name"] == "[Multi-day 3D Point Cloud] Surface Change"
    C = np.asarray(model["centers"], np.float32)
    np.testing.assert_array_equal(data, C.astype(np.float64))
    props = params["properties"]
    assert set(props) == {"count", "dz", "rms"}
    X = clouds[2].astype(np.float32)
    q = R.fixed_q(X)
    Xd = dequantised(X, q)
    labels = res["labels"]
    np.testing.assert_array_equal(props["count"], np.bincount(labels, minlength=k))
    assert (props["count"] == 0).any() and (props["count"] > 0).any()       # the third day misses the right half
    for j in range(k):
        P = Xd[labels == j]
        if P.shape[0] == 0:
            assert props["dz"][j] == 0.0 and props["rms"][j] == 0.0
            continue
        assert props["dz"][j] == pytest.approx(P[:, 0].mean() - float(C[j, 0]), rel=1e-9, abs=1e-12)
        assert props["rms"][j] == pytest.approx(np.sqrt(np.var(P, axis=0).sum()), rel=1e-7, abs=1e-9)
    assert np.median(props["dz"][props["count"] > 50]) > 0.2                # the third day sits 0.5 higher
    assert res["stats"]["words"].shape == (1, k, 16) and res["stats"]["sizes"] == [X.shape[0]]


def test_extractor_passes_describe():
    from fake_pipeline import SyntheticPairExtractor
    import pcm_amd
    base = SyntheticPairExtractor(n_pairs=2, shape=(40, 50))
    plain = pcm_amd.HeightMapExtractor(base=base, n_clusters=8, fit=oracle_fit_plugin)
    out0 = plain.run("roi.kml")
    assert set(out0[-2][1]["properties"]) == {"height", "count"} and "stats" not in plain.last_result
    ext = pcm_amd.HeightMapExtractor(base=base, n_clusters=8, fit=oracle_fit_plugin, describe=True, stats=oracle_stats)
    out = ext.run("roi.kml")
    assert len(out) == len(out0)
    assert {"roughness", "normal_z", "days_seen", "height_spread"} <= set(out[-2][1]["properties"])
    assert (out[-2][1]["properties"]["days_seen"] <= 2).all() and "stats" in ext.last_result
    model = ext.last_result
    asg = pcm_amd.HeightMapExtractor(base=base, model=model, assign=oracle_assign, describe=True, stats=oracle_stats)
    out2 = asg.run("roi.kml")
    assert [l[1]["name"] for l in out2][-2:] == ["[Multi-day 3D Point Cloud] Assigned 3D Point Cloud",
                                                 "[Multi-day 3D Point Cloud] Surface Change"]
    asg0 = pcm_amd.HeightMapExtractor(base=base, model=model, assign=oracle_assign)
    assert len(asg0.run("roi.kml")) == len(out2) - 1 and set(asg0.last_result) == {"labels", "distance", "inertia",
                                                                                   "n_points"}
