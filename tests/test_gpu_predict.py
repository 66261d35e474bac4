"""GPU: ``pcm_predict`` (the sort-free pruned E-step for given centres),
``pcm_dense_predict`` / ``pcm_dense_transform`` and everything built on them,
bitwise against the CPU oracle:

* labels      = ``R.assign(X, C)``
* sq. dist.   = ``R.sqdist_rows(X, C[labels])``
* inertia     = ``R.inertia_exact(dist, R.inertia_scale(R.fixed_q(vstack([X, C]))))``
* dense       = ``DR.assign`` / ``DR.inertia_exact`` with ``DR.inertia_scale(maxabs over X and C)``
* transform   = ``np.sqrt(DR.sqdist(X, C))`` (IEEE sqrt is correctly rounded on both sides)

``info`` (cells, FULL cells, summed list length) tells which path labelled the points.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import dense_ref as DR  # noqa: E402
from oracle import lloyd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def pcm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pcm_amd
    from pcm_amd import _lib
    _lib.load()
    return pcm_amd


def oracle(X, C):
    X = np.ascontiguousarray(X, np.float32)
    C = np.ascontiguousarray(C, np.float32)
    labels = R.assign_fast(X, C) if X.shape[0] else np.zeros(0, np.int32)
    sq = R.sqdist_rows(X, C[labels]) if X.shape[0] else np.zeros(0, np.float32)
    return labels, sq, R.inertia_exact(sq, R.inertia_scale(R.fixed_q(np.vstack([X, C]))))


def run(pcm, X, C, dtype=torch.float32):
    Xt = torch.from_numpy(np.ascontiguousarray(X)).to("cuda", dtype)
    res = pcm.lloyd_predict(Xt, torch.from_numpy(np.ascontiguousarray(C, np.float32)).cuda(), return_distance=True,
                            return_inertia=True)
    torch.cuda.synchronize()
    return res


def check(pcm, X, C, dtype=torch.float32, where=""):
    res = run(pcm, X, C, dtype)
    labels, sq, inertia = oracle(X, C)
    got = res.labels.cpu().numpy()
    print(f"{where} n={X.shape[0]} k={C.shape[0]} d={X.shape[1]} info={res.info} inertia={res.inertia!r}")
    bad = np.flatnonzero(got != labels)
    assert got.dtype == np.int32 and bad.size == 0, f"{where} {bad.size} labels differ, first rows {bad[:8]}"
    gd = res.distance.cpu().numpy()
    assert gd.dtype == np.float32 and np.array_equal(gd.view(np.uint32), sq.view(np.uint32)), f"{where} distances differ"
    assert res.inertia == inertia, f"{where} inertia {res.inertia!r} != {inertia!r}"
    return res


def blobs(n, d, seed, nb=12, sd=0.8):
    rng = np.random.default_rng(seed)
    centers = rng.random((nb, d)) * 10
    return (centers[rng.integers(0, nb, n)] + rng.normal(0, sd, (n, d))).astype(np.float32)


# ---------------------------------------------------------------- 1. blobs
# A cell's list holds every centre that its reference centre does not dominate
# over the whole cell.  In a void between a few large blobs all the centres of
# the blobs around it are about equally far, so a void cell's list grows with
# the centres per blob (K / 12 here); a 4-D cell has 80 neighbours against 26 in
# 3-D, and at K = 256 some void cells of 12 blobs then pass CAPF = 64 whatever the
# blobs' width (test_blobs_4d_void_cells).  With many small blobs (about one per
# centre) a void is contested only by the centres next to it: the D = 4 cases use
# 2000 blobs of sigma 0.3, whose longest list stays below 50.
@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("k", [8, 64, 256])
def test_blobs(pcm, k, d):
    n = 50_000
    X = blobs(n, d, 100 * d + k) if d < 4 else blobs(n, d, 100 * d + k, nb=2000, sd=0.3)
    C = X[R.init_indices(n, k)]
    res = check(pcm, X, C, where="blobs")
    assert res.info["cells"] > 1 and res.info["full_cells"] == 0
    assert res.info["mean_list"] < k          # pruning ran
    # labels and distances do not depend on which outputs are asked for
    Xt, Ct = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    only = pcm.lloyd_predict(Xt, Ct)
    assert only.distance is None and only.inertia is None
    assert torch.equal(only.labels, res.labels)
    # nor on q: other exponents move the inertia scale only
    other = pcm.lloyd_predict(Xt, Ct, return_distance=True, return_inertia=True, q=[0] * d)
    assert torch.equal(other.labels, res.labels) and torch.equal(other.distance, res.distance)
    sq = other.distance.cpu().numpy()
    assert other.inertia == R.inertia_exact(sq, R.inertia_scale([0] * d))


def test_blobs_4d_void_cells(pcm):
    """12 large blobs in D = 4 at K = 256: a handful of (nearly empty) void cells
    between the blobs have more than CAPF candidates and scan all K (9 of 5832
    cells on record, holding a handful of the 50 000 points); most cells are pruned and
    every label, distance and the inertia stay bitwise."""
    n, k = 50_000, 256
    X = blobs(n, 4, 656)
    res = check(pcm, X, X[R.init_indices(n, k)], where="blobs 4-D voids")
    assert res.info["full_cells"] < res.info["cells"] // 100 and res.info["mean_list"] < 64


# ---------------------------------------------------------------- 2. fp16, D = 4
def test_fp16_d4_golden(pcm):
    g = np.load(os.path.join(GOLDEN, "d4_fp16.npz"))
    X = g["X"]
    assert np.array_equal(X.astype(np.float16).astype(np.float32), X)      # widened exactly
    check(pcm, X, g["C0"], dtype=torch.float16, where="d4_fp16 C0")
    check(pcm, X, g["fit_centers"], dtype=torch.float16, where="d4_fp16 fit")


# ---------------------------------------------------------------- 3. ties and duplicates
def test_ties_and_duplicates(pcm):
    g = np.load(os.path.join(GOLDEN, "ties_dups.npz"))
    for t in range(g["c_in"].shape[0]):
        res = check(pcm, g["X"], g["c_in"][t], where=f"ties_dups {t}")
        np.testing.assert_array_equal(res.labels.cpu().numpy(), g["labels"][t])     # sklearn's labels


def test_lattice_ties_lowest_index_wins(pcm):
    ax = np.arange(16, dtype=np.float32)
    X = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    X = np.concatenate([X, X[::7]])                                             # duplicates
    mid = np.arange(0.5, 15, 1.0, dtype=np.float32)                             # lattice midpoints: 8-way ties
    C = np.stack(np.meshgrid(mid, mid, mid, indexing="ij"), axis=-1).reshape(-1, 3)
    C = np.concatenate([C[:100], C[40:41], C[100:], C[7:8]])                    # two pairs of identical centres
    res = check(pcm, X, C, where="lattice")
    lab = res.labels.cpu().numpy()
    assert not np.isin(lab, [100, C.shape[0] - 1]).any()                        # the later twin never wins
    d = R.sqdist(X, C)
    ties = (d == d.min(axis=1, keepdims=True)).sum(axis=1)
    assert (ties >= 2).sum() > 1000                                             # the case is about ties
    np.testing.assert_array_equal(lab, np.argmin(d, axis=1))


# ---------------------------------------------------------------- 4. FULL cells
def test_full_cells_scan_all_centres(pcm):
    n, k = 20_000, 256
    X = R.splitmix_uniform(n, 3, seed=21)
    rng = np.random.default_rng(4)
    v = rng.normal(size=(k, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.random((k, 1)) * 1e-6
    C = (0.5 + v).astype(np.float32)
    assert np.unique(C, axis=0).shape[0] > 64
    res = check(pcm, X, C, where="full")
    assert res.info["full_cells"] >= 1


# ---------------------------------------------------------------- 5. centres outside the box of X
def test_centres_far_outside_the_cloud(pcm):
    X = R.splitmix_uniform(30_000, 3, seed=5)
    C = (np.random.default_rng(6).random((64, 3)) * 100 - 50).astype(np.float32)
    res = check(pcm, X, C, where="centres outside")
    assert np.isfinite(res.inertia)
    # the exponents of X alone cannot hold these distances: the default covers the centres too
    assert not np.isfinite(R.inertia_exact(res.distance.cpu().numpy(), R.inertia_scale(R.fixed_q(X))))


def test_cloud_far_outside_the_centres(pcm):
    X = (R.splitmix_uniform(30_000, 3, seed=8) * 100 - 50).astype(np.float32)
    C = R.splitmix_uniform(64, 3, seed=9)
    res = check(pcm, X, C, where="cloud outside")
    assert np.isfinite(res.inertia)


# ---------------------------------------------------------------- 6. degenerate shapes
def test_degenerate_shapes(pcm):
    X = R.splitmix_uniform(50_001, 3, seed=3)                       # not a multiple of 4, 64 or the block
    C = X[R.init_indices(50_001, 32)]
    check(pcm, X, C, where="n=50001")
    Xc = X.copy()
    Xc[:, 1] = 2.5                                                  # one axis constant
    check(pcm, Xc, Xc[R.init_indices(50_001, 32)], where="constant axis")
    check(pcm, Xc, C, where="constant axis, centres off it")
    res = check(pcm, X[:5000], C[:1], where="k=1")                  # no lists
    assert res.info["cells"] == 0
    check(pcm, X[:1], C, where="n=1")
    check(pcm, X[:3], C[:2], where="n=3")
    # points exactly on the upper faces of the box
    F = X[:4096].copy()
    F[::3, 0] = F[:, 0].max()
    F[1::5, 1] = F[:, 1].max()
    F[2::7, 2] = F[:, 2].max()
    F[::11] = F.max(axis=0)
    check(pcm, F, C, where="upper faces")
    for d in (1, 2, 4):
        Y = R.splitmix_uniform(1237, d, seed=d)
        check(pcm, Y, Y[R.init_indices(1237, 40)], where=f"d={d} small")


# Thin, non-degenerate boxes: one axis far shorter than the others but not
# constant.  make_grid sizes cells from the volume and keeps one cell on the thin
# axis, so the long axes get far more cells than the target at any target; the
# grid is then cut down to the workspace bounds (n, k, extents per axis).
THIN = [
    (1000, 8, (1, 1e-4, 1)),
    (50_001, 32, (1, 1e-6, 1)),
    (3, 2, (1000, 1, 0.001)),
    (2000, 8, (100, 0.001)),
    (100, 8, (1, 1, 1, 1e-5)),
    (20_000, 64, (1, 1, 1e-5, 1)),
    (5000, 16, (1e-3, 50)),
]


@pytest.mark.parametrize("n,k,ext", THIN, ids=[f"n{n}-k{k}-d{len(e)}" for n, k, e in THIN])
def test_thin_clouds(pcm, n, k, ext):
    d = len(ext)
    X = (R.splitmix_uniform(n, d, seed=n + d) * np.asarray(ext, np.float32)).astype(np.float32)
    assert (X.max(axis=0) > X.min(axis=0)).all()                    # no axis is constant
    C = X[R.init_indices(n, k)]
    res = check(pcm, X, C, where=f"thin {ext}")
    assert 1 <= res.info["cells"] <= 1.5 * max(1.0, min((48 if d == 4 else 32) * k, n / 8)) + 16
    off = (R.splitmix_uniform(k, d, seed=77) * 2 - 0.5).astype(np.float32)
    check(pcm, X, off, where=f"thin {ext}, centres off the slab")


def test_almost_constant_axis(pcm):
    """The constant-axis cloud with a few ulp of noise on that axis."""
    X = R.splitmix_uniform(50_001, 3, seed=3)
    noise = np.random.default_rng(1).integers(-2, 3, X.shape[0]).astype(np.float32) * np.float32(2.0 ** -22)
    X[:, 1] = np.float32(2.5) + noise
    assert np.unique(X[:, 1]).size == 5
    check(pcm, X, X[R.init_indices(50_001, 32)], where="almost constant axis")


def test_empty_cloud(pcm):
    C = R.splitmix_uniform(8, 3, seed=1)
    res = pcm.lloyd_predict(torch.empty((0, 3), device="cuda"), torch.from_numpy(C).cuda(), return_distance=True,
                            return_inertia=True)
    assert res.labels.shape == (0,) and res.labels.dtype == torch.int32
    assert res.distance.shape == (0,) and res.inertia == 0.0


# ---------------------------------------------------------------- 7. a larger cloud
def test_larger_cloud_against_device_bruteforce(pcm):
    from pcm_amd.engine import assign_bruteforce, synth_uniform
    n, k = 200_000, 1024
    Xt = synth_uniform(n, 3, seed=11)
    idx = R.init_indices(n, k)
    Ct = Xt[torch.from_numpy(idx).cuda()].contiguous()
    res = pcm.lloyd_predict(Xt, Ct, return_distance=True, return_inertia=True)
    want = assign_bruteforce(Xt, Ct, [25, 25, 25])                 # no statistics: q is unused
    torch.cuda.synchronize()
    print("larger", res.info)
    assert torch.equal(res.labels, want)
    assert res.info["full_cells"] == 0 and res.info["mean_list"] < 64
    rows = np.sort(np.random.default_rng(0).choice(n, 20_000, replace=False))
    X, C = Xt.cpu().numpy(), Ct.cpu().numpy()
    labels, sq, _ = oracle(X[rows], C)
    np.testing.assert_array_equal(res.labels.cpu().numpy()[rows], labels)
    assert np.array_equal(res.distance.cpu().numpy()[rows].view(np.uint32), sq.view(np.uint32))


# ---------------------------------------------------------------- 8. errors
def test_errors(pcm):
    from pcm_amd._lib import PcmError
    X = R.splitmix_uniform(1000, 3, seed=2)
    C = X[:8].copy()
    bad = X.copy()
    bad[777, 2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        pcm.lloyd_predict(torch.from_numpy(bad).cuda(), torch.from_numpy(C).cuda())
    bad[777, 2] = np.inf
    with pytest.raises(ValueError):
        pcm.lloyd_predict(torch.from_numpy(bad).cuda(), torch.from_numpy(C).cuda(), return_inertia=True)
    Cb = C.copy()
    Cb[3, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        pcm.lloyd_predict(torch.from_numpy(X).cuda(), torch.from_numpy(Cb).cuda())
    with pytest.raises(PcmError):
        pcm.lloyd_predict(torch.from_numpy(X), torch.from_numpy(C))              # host tensor: no CPU fallback
    with pytest.raises(ValueError):
        pcm.lloyd_predict(torch.from_numpy(X).cuda(), torch.from_numpy(C[:, :2].copy()).cuda())
    with pytest.raises(PcmError):
        pcm.dense_predict(torch.from_numpy(X), torch.from_numpy(C))
    with pytest.raises(ValueError):
        pcm.dense_predict(torch.from_numpy(bad).cuda(), torch.from_numpy(C).cuda())
    with pytest.raises(ValueError):
        pcm.dense_transform(torch.from_numpy(X).cuda(), torch.from_numpy(Cb).cuda())


# ---------------------------------------------------------------- 9. dense
DENSE = [  # n, d, k: the reference call-site shape; a wider K; centres beyond the 64 KB LDS stage (float64);
    (1500, 20, 5), (4000, 8, 32), (300, 64, 200), (37, 2, 5000)]   # K > one chunk of outputs per row


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,d,k", DENSE)
def test_dense_predict_and_transform(pcm, n, d, k, dtype):
    rng = np.random.default_rng(n + d + k)
    X = rng.normal(0, 2.0, (n, d)).astype(dtype)
    C = (X[rng.integers(0, n, k)] + rng.normal(0, 0.5, (k, d))).astype(dtype)
    C[0] *= 40                                                     # a centre well outside the rows' range
    Xt, Ct = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    res = pcm.dense_predict(Xt, Ct, return_distance=True, return_inertia=True)
    labels, sq = DR.assign(X, C)
    np.testing.assert_array_equal(res.labels.cpu().numpy(), labels)
    gd = res.distance.cpu().numpy()
    assert gd.dtype == dtype and np.array_equal(gd, sq)
    assert res.inertia == DR.inertia_exact(sq, DR.inertia_scale(np.abs(np.vstack([X, C])).max(axis=0)))
    only = pcm.dense_predict(Xt, Ct)
    assert only.distance is None and only.inertia is None and torch.equal(only.labels, res.labels)
    T = pcm.dense_transform(Xt, Ct).cpu().numpy()
    want = np.sqrt(DR.sqdist(X, C))
    assert T.dtype == dtype and T.shape == (n, k)
    bad = np.flatnonzero(T != want)
    assert bad.size == 0, f"{bad.size} of {T.size} distances differ from the correctly rounded sqrt"


def _held_out(est, ref, Y):
    np.testing.assert_array_equal(est.cluster_centers_, ref.cluster_centers_)
    np.testing.assert_array_equal(est.predict(Y), ref.predict(Y))
    np.testing.assert_array_equal(est.transform(Y), ref.transform(Y))
    assert est.score(Y) == ref.score(Y)
    np.testing.assert_array_equal(est.fit_transform(Y[:500]), est.transform(Y[:500]))


def test_estimator_apply_point_cloud(pcm):
    from test_estimator import cloud, oracle_fit, oracle_seed
    from test_predict import oracle_predict, oracle_transform
    XY = cloud(8000, 3, 42)
    X, Y = XY[:4000], XY[4000:]
    est = pcm.KMeans(n_clusters=8, random_state=42, n_init=1).fit(X)
    ref = pcm.KMeans(n_clusters=8, random_state=42, n_init=1, _fit=oracle_fit, _seed=oracle_seed,
                     _predict=oracle_predict, _transform=oracle_transform).fit(X)
    _held_out(est, ref, Y)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_estimator_apply_dense(pcm, dtype):
    from test_dense import oracle_fit, oracle_seed
    from test_predict import oracle_predict, oracle_transform
    rng = np.random.default_rng(3)
    XY = (rng.normal(0, 1, (3000, 20)) + 3 * rng.integers(0, 3, (3000, 1))).astype(dtype)
    X, Y = XY[:1500], XY[1500:]
    est = pcm.KMeans(n_clusters=5, random_state=42, n_init=1).fit(X)
    ref = pcm.KMeans(n_clusters=5, random_state=42, n_init=1, _fit=oracle_fit, _seed=oracle_seed,
                     _predict=oracle_predict, _transform=oracle_transform).fit(X)
    _held_out(est, ref, Y)


# ---------------------------------------------------------------- 10. plugin
def test_plugin_assign_matches_oracle(pcm):
    from test_predict import oracle_assign
    g = np.load(os.path.join(GOLDEN, "plugin", "plugin_cloud_k64.npz"))
    X = g["X"].astype(np.float64)
    model = dict(centers=g["f32_centers"])
    clouds = [X[:30_000], X[30_000:]]
    layers, res = pcm.kmeans_assign(clouds, model)
    layers_o, want = pcm.kmeans_assign(clouds, model, assign=oracle_assign)
    np.testing.assert_array_equal(res["labels"], want["labels"])
    np.testing.assert_array_equal(res["distance"], want["distance"])
    assert res["inertia"] == want["inertia"] and res["n_points"] == X.shape[0]
    for key in ("cluster", "residual", "height"):
        np.testing.assert_array_equal(layers[0][1]["properties"][key], layers_o[0][1]["properties"][key])
    # the device_clouds shortcut reads the same points on the GPU
    dev = [torch.from_numpy(c).cuda() for c in clouds]
    _, res_d = pcm.kmeans_assign(clouds, model, device_clouds=dev)
    np.testing.assert_array_equal(res_d["labels"], want["labels"])
    np.testing.assert_array_equal(res_d["distance"], want["distance"])
    # on the cloud the model was fitted to, the labels are the fit's own
    np.testing.assert_array_equal(res["labels"], g["f32_labels"])
