"""CPU: applying a fitted model -- ``KMeans.predict / transform / fit_transform /
score`` (sklearn 1.7.2 semantics, ``sklearn/cluster/_kmeans.py:1067-1191``), the
plugin's ``kmeans_assign`` / ``HeightMapExtractor(model=...)`` and the argument
checks of the predict ABI.  The device legs are replaced by the oracle through
the constructor stand-ins (the product has no CPU fallback); the HIP kernels
are checked in tests/test_gpu_predict.py.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

from oracle import dense_ref as DR
from oracle import lloyd_ref as R
from test_estimator import cloud, oracle_fit, oracle_seed


def oracle_predict(X, C):
    """The semantics pcm_predict / pcm_dense_predict hold: canonical labels, squared
    distances to the winners and the exact inertia with exponents over X and C."""
    if X.dtype == np.float32 and X.shape[1] <= 4:
        labels = R.assign(X, C)
        sq = R.sqdist_rows(X, C[labels])
        return labels, sq, R.inertia_exact(sq, R.inertia_scale(R.fixed_q(np.vstack([X, C]))))
    labels, sq = DR.assign(X, C)
    return labels, sq, DR.inertia_exact(sq, DR.inertia_scale(np.abs(np.vstack([X, C])).max(axis=0)))


def oracle_transform(X, C):
    return np.sqrt(DR.sqdist(X, C))


def estimator(k, seed, **kw):
    import pcm_amd
    return pcm_amd.KMeans(n_clusters=k, random_state=seed, n_init=1, _fit=oracle_fit, _seed=oracle_seed,
                          _predict=oracle_predict, _transform=oracle_transform, **kw)


# ---------------------------------------------------------------- estimator control flow
def test_apply_before_fit_raises():
    est = estimator(4, 0)
    X = cloud(50, 3, 0)
    for call in (est.predict, est.transform, est.score):
        with pytest.raises((ValueError, AttributeError)):
            call(X)


def test_wrong_feature_count_and_nan_raise():
    est = estimator(4, 0).fit(cloud(400, 3, 0))
    for call in (est.predict, est.transform, est.score):
        with pytest.raises(ValueError, match="features"):
            call(cloud(10, 2, 1))
        bad = cloud(10, 3, 1)
        bad[3, 1] = np.nan
        with pytest.raises(ValueError, match="NaN"):
            call(bad)
        bad[3, 1] = np.inf
        with pytest.raises(ValueError):
            call(bad)
    with pytest.raises(NotImplementedError):
        est.score(cloud(10, 3, 1), sample_weight=np.full(10, 2.0))
    assert est.score(cloud(10, 3, 1), sample_weight=np.ones(10)) <= 0.0


def test_fit_transform_equals_fit_then_transform():
    X = cloud(600, 3, 5)
    a = estimator(6, 3).fit_transform(X)
    est = estimator(6, 3).fit(X)
    b = est.transform(X)
    np.testing.assert_array_equal(a, b)
    assert a.shape == (600, 6) and a.dtype == np.float32
    np.testing.assert_array_equal(b, np.sqrt(DR.sqdist(X, est.cluster_centers_)))
    # the nearest column of transform is predict's label (distances are monotone in their squares)
    np.testing.assert_array_equal(np.argmin(b.astype(np.float64) ** 2, axis=1), np.argmin(DR.sqdist(X, est.cluster_centers_), axis=1))


def test_score_is_minus_inertia_of_x():
    X, Y = cloud(800, 3, 2), cloud(300, 3, 9)
    est = estimator(5, 1).fit(X)
    for Z in (X, Y):
        labels = est.predict(Z)
        np.testing.assert_array_equal(labels, R.assign(Z, est.cluster_centers_))
        sq = R.sqdist_rows(Z, est.cluster_centers_[labels])
        want = R.inertia_exact(sq, R.inertia_scale(R.fixed_q(np.vstack([Z, est.cluster_centers_]))))
        assert est.score(Z) == -want
    # on the training rows that is the fit's inertia up to the centring round trip (sklearn likewise)
    assert est.score(X) == pytest.approx(-float(est.inertia_), rel=1e-4)
    # a stand-in without an inertia: the float64 sum of the squared distances
    import pcm_amd
    est2 = pcm_amd.KMeans(n_clusters=5, random_state=1, n_init=1, _fit=oracle_fit, _seed=oracle_seed,
                          _predict=lambda Z, C: oracle_predict(Z, C)[:2]).fit(X)
    assert est2.score(Y) == -float(np.sum(R.sqdist_rows(Y, est2.cluster_centers_[est2.predict(Y)]), dtype=np.float64))


def test_predict_is_not_centred():
    """predict uses X as given against cluster_centers_: shifting X and the centres
    by the same exactly representable offset keeps every label."""
    rng = np.random.default_rng(11)
    X = (rng.integers(0, 1024, (500, 3)) / 8.0).astype(np.float32)     # multiples of 1/8 below 128
    est = estimator(7, 4).fit(X)
    C = (np.round(est.cluster_centers_ * 8) / 8).astype(np.float32)
    est.cluster_centers_ = C
    base = est.predict(X)
    np.testing.assert_array_equal(base, R.assign(X, C))
    off = np.float32(4096.0)                                           # X + off, C + off exact in float32
    assert np.array_equal((X + off) - off, X) and np.array_equal((C + off) - off, C)
    est.cluster_centers_ = C + off
    np.testing.assert_array_equal(est.predict(X + off), base)
    # whereas a predict that centred X by its own mean would label Xs = X + (0, 0, 64) as X
    Xs = X + np.float32([0, 0, 64])
    np.testing.assert_array_equal(est.predict(Xs + off), R.assign(Xs + off, C + off))
    assert not np.array_equal(est.predict(Xs + off), base)


def test_float64_rows_use_the_dense_semantics():
    X = cloud(300, 3, 3).astype(np.float64)
    est = estimator(4, 2).fit(X)
    assert est.cluster_centers_.dtype == np.float64
    labels = est.predict(X[:100])
    np.testing.assert_array_equal(labels, DR.assign(X[:100], est.cluster_centers_)[0])
    assert est.transform(X[:100]).dtype == np.float64
    # float32 rows against a float64 model: the centres are taken in X's precision
    l32 = est.predict(X[:100].astype(np.float32))
    np.testing.assert_array_equal(l32, R.assign(X[:100].astype(np.float32), est.cluster_centers_.astype(np.float32)))


# ---------------------------------------------------------------- scikit-learn
SK_CASES = [(3000, 8, 3, 42), (4096, 32, 3, 7), (2000, 6, 2, 1), (5000, 16, 4, 0)]   # n, k, d, seed


@pytest.mark.parametrize("n,k,d,seed", SK_CASES)
def test_apply_matches_sklearn(n, k, d, seed):
    sk = pytest.importorskip("sklearn.cluster")
    XY = cloud(2 * n, d, seed)
    X, Y = XY[:n], XY[n:]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = sk.KMeans(n_clusters=k, random_state=seed, n_init=1).fit(X)
    est = estimator(k, seed).fit(X)
    np.testing.assert_array_equal(est.labels_, ref.labels_)
    np.testing.assert_array_equal(est.predict(Y), ref.predict(Y))
    np.testing.assert_allclose(est.transform(Y), ref.transform(Y), rtol=1e-5, atol=1e-5 * float(np.abs(Y).max()))
    assert est.score(Y) == pytest.approx(ref.score(Y), rel=1e-4)


# ---------------------------------------------------------------- plugin
def oracle_assign(X, C):
    return oracle_predict(np.ascontiguousarray(X, np.float32), np.ascontiguousarray(C, np.float32))


def oracle_fit_plugin(X, C0, max_iter, tol_abs):
    r = R.lloyd_fit(X, C0, max_iter=max_iter, tol=tol_abs)
    return r["labels"], r["centers"], r["inertia"], r["n_iter"]


def _two_days():
    from fake_pipeline import SyntheticPairExtractor
    import pcm_amd
    day1 = [l[0] for l in SyntheticPairExtractor(n_pairs=2, shape=(40, 50)).run("roi.kml") if l[2] == "points"]
    day2 = [l[0] for l in SyntheticPairExtractor(n_pairs=1, shape=(36, 44)).run("roi.kml") if l[2] == "points"]
    _, model = pcm_amd.kmeans_fuse(day1, n_clusters=8, fit=oracle_fit_plugin)
    return day1, day2, model


def test_kmeans_assign_layer_and_result(tmp_path):
    import pcm_amd
    day1, day2, model = _two_days()
    layers, res = pcm_amd.kmeans_assign(day2, model, assign=oracle_assign)
    assert len(layers) == 1
    data, params, kind = layers[0]
    assert kind == "points" and params["name"] == "[Multi-day 3D Point Cloud] Assigned 3D Point Cloud"
    X = np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in day2]).astype(np.float32)
    C = np.asarray(model["centers"], np.float32)
    n = X.shape[0]
    assert data.shape == (n, 3) and data.dtype == np.float64 and res["n_points"] == n
    props = params["properties"]
    assert set(props) == {"cluster", "residual", "height"}
    assert props["cluster"].dtype == np.int32 and props["residual"].dtype == np.float64
    assert props["height"].dtype == np.float64 and props["height"].shape == (n,)
    assert 0.0 <= props["height"].min() and props["height"].max() <= 1.0
    want = R.assign(X, C)
    np.testing.assert_array_equal(props["cluster"], want)
    np.testing.assert_array_equal(props["residual"], np.sqrt(R.sqdist_rows(X, C[want]).astype(np.float64)))
    np.testing.assert_array_equal(res["labels"], want)
    np.testing.assert_array_equal(res["distance"], props["residual"])
    assert res["inertia"] == oracle_assign(X, C)[2]
    # the model as an export_fused file gives the same result as the dict
    path = str(tmp_path / "model.npz")
    Xfit = np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in day1])
    pcm_amd.plugin.export_fused(path, Xfit, model)
    for m in (path, pcm_amd.plugin.load_fused(path)):
        layers2, res2 = pcm_amd.kmeans_assign(day2, m, assign=oracle_assign)
        np.testing.assert_array_equal(res2["labels"], res["labels"])
        np.testing.assert_array_equal(res2["distance"], res["distance"])
        assert res2["inertia"] == res["inertia"]
        np.testing.assert_array_equal(layers2[0][0], data)
    with pytest.raises(ValueError):
        pcm_amd.kmeans_assign([], model, assign=oracle_assign)


def test_extractor_model_mode():
    from fake_pipeline import SyntheticPairExtractor, SyntheticStages
    from test_plugin import oracle_assemble
    import pcm_amd
    _, _, model = _two_days()
    base = SyntheticPairExtractor(n_pairs=2, shape=(40, 50))
    ref_layers = base.run("roi.kml")
    # model=None (the default): the fused output is what it was
    fused = pcm_amd.HeightMapExtractor(base=base, n_clusters=8, fit=oracle_fit_plugin).run("roi.kml")
    assert [l[1]["name"] for l in fused][-2:] == ["[Multi-day 3D Point Cloud] Fused K-means Centroids",
                                                  "[Multi-day 3D Point Cloud] Fused 3D Point Cloud"]
    assert len(fused) == len(ref_layers) + 2
    # model given: nothing is fused, one assigned layer is appended
    plugin = pcm_amd.HeightMapExtractor(base=base, model=model, assign=oracle_assign)
    out = plugin.run("roi.kml")
    assert len(out) == len(ref_layers) + 1
    assert out[-1][1]["name"] == "[Multi-day 3D Point Cloud] Assigned 3D Point Cloud"
    assert not any("Fused" in l[1]["name"] for l in out)
    clouds = [l[0] for l in ref_layers if l[2] == "points"]
    _, want = pcm_amd.kmeans_assign(clouds, model, assign=oracle_assign)
    np.testing.assert_array_equal(plugin.last_result["labels"], want["labels"])
    np.testing.assert_array_equal(out[-1][1]["properties"]["cluster"], want["labels"])
    assert set(plugin.last_result) == {"labels", "distance", "inertia", "n_points"}
    # the GPU-stages path takes the same branch
    st = pcm_amd.HeightMapExtractor(stages=SyntheticStages(n_pairs=2, shape=(40, 50)), model=model,
                                    assign=oracle_assign, _assemble=oracle_assemble)
    out2 = st.run("roi.kml")
    assert out2[-1][1]["name"] == "[Multi-day 3D Point Cloud] Assigned 3D Point Cloud"
    assert not any("Fused" in l[1]["name"] for l in out2)
    assert st.last_result["n_points"] == out2[-1][0].shape[0]
    # errors keep the error-layer convention
    def boom(X, C):
        raise RuntimeError("HIP extension missing")
    err = pcm_amd.HeightMapExtractor(base=base, model=model, assign=boom).run("roi.kml")
    assert len(err) == 1 and err[0][2] == "image" and err[0][1]["name"].startswith("Error:")


# ---------------------------------------------------------------- ABI
def test_predict_argument_errors_without_device():
    """The argument checks of the predict entry points run before any device call."""
    from pcm_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    lib = _lib.load(require_gpu_runtime=False)
    nb = ctypes.c_size_t()
    one = ctypes.c_void_p(256)      # a non-null address that is never dereferenced
    assert lib.pcm_predict(None, 0, 10, 3, one, 4, None, one, None, None, None, one, 1 << 20, None) == -1   # NULL X
    assert "null" in _lib.last_error()
    assert lib.pcm_predict(one, 0, 10, 5, one, 4, None, one, None, None, None, one, 1 << 20, None) == -1    # d = 5
    assert "d must be" in _lib.last_error()
    assert lib.pcm_predict(one, 0, 10, 3, one, 0, None, one, None, None, None, one, 1 << 20, None) == -1    # k < 1
    assert lib.pcm_predict(one, 2, 10, 3, one, 4, None, one, None, None, None, one, 1 << 20, None) == -1    # float64
    assert lib.pcm_predict_workspace(10, 5, 4, ctypes.byref(nb)) == -1
    assert lib.pcm_predict_workspace(10, 3, 0, ctypes.byref(nb)) == -1
    assert lib.pcm_predict_workspace(100_000, 3, 64, ctypes.byref(nb)) == 0 and nb.value > 0
    small = nb.value
    assert lib.pcm_predict_workspace(100_000_000, 3, 1024, ctypes.byref(nb)) == 0 and nb.value > small
    assert lib.pcm_dense_predict(None, 0, 10, 8, one, 4, None, one, None, None, one, 256, None) == -1       # NULL X
    assert lib.pcm_dense_predict(one, 0, 10, 65, one, 4, None, one, None, None, one, 256, None) == -1       # d > 64
    assert lib.pcm_dense_predict(one, 0, 10, 8, one, 0, None, one, None, None, one, 256, None) == -1        # k < 1
    assert lib.pcm_dense_predict(one, 1, 10, 8, one, 4, None, one, None, None, one, 256, None) == -1        # float16
    assert lib.pcm_dense_transform(one, 0, 10, 8, one, 4, None, None) == -1                                 # NULL out
    assert lib.pcm_dense_transform(one, 0, 10, 0, one, 4, one, None) == -1                                  # d < 1


def test_public_names():
    import pcm_amd
    for name in ("lloyd_predict", "LloydPrediction", "dense_predict", "dense_transform", "kmeans_assign"):
        assert name in pcm_amd.__all__
    from pcm_amd import _lib
    assert _lib.ABI_VERSION == 8
    for name in ("pcm_predict", "pcm_predict_workspace", "pcm_dense_predict", "pcm_dense_transform"):
        assert name in _lib.EXPORTS
