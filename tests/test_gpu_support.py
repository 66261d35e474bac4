"""GPU: ``radius_support`` / ``filter_outliers`` and the plugin's ``denoise=``, every output bitwise
against the NumPy brute force (tests/support_ref.py): whichever cells, runs and chunks the kernel
walks, the counts and days are the same integers.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import support_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

LATTICE_RADII = (0.75, 1.25, 2.5)


@pytest.fixture(scope="module")
def pcm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pcm_amd
    from pcm_amd import _lib
    _lib.load()
    return pcm_amd


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def run(pcm, X, r, groups=None, n_groups=None, max_count=None):
    sup = pcm.radius_support(dev(X, np.float32), r, groups=None if groups is None else dev(groups),
                             n_groups=n_groups, max_count=max_count)
    torch.cuda.synchronize()
    return sup, sup.counts.cpu().numpy(), None if sup.days is None else sup.days.cpu().numpy()


def check(pcm, X, r, groups=None, n_groups=None, max_count=None):
    """The kernel against the brute force; -> (Support, the reference's uncapped counts)."""
    want_c, want_d, want_s = S.brute(X, r, groups, n_groups, max_count)
    sup, counts, days = run(pcm, X, r, groups, n_groups, max_count)
    assert counts.dtype == np.int32 and np.array_equal(counts, want_c)
    if groups is None:
        assert days is None
    else:
        assert days.dtype == np.int32 and np.array_equal(days, want_d)
    assert sup.skipped == want_s and sup.radius == float(np.float32(r))
    return sup, want_c


@pytest.fixture(scope="module")
def lattice():
    X = S.lattice_cloud(3000, 5)
    return X, np.random.default_rng(11).integers(0, 3, X.shape[0])


@pytest.mark.parametrize("r", LATTICE_RADII)
def test_lattice(pcm, lattice, r):
    X, groups = lattice
    sup, _ = check(pcm, X, r)
    assert sup.cell_log2 == S.plan(X, r)[0]
    check(pcm, X, r, groups, 3)


def test_general_floats(pcm):
    rng = np.random.default_rng(3)
    X = (rng.random((4096, 3)) * np.array([8.0, 64.0, 64.0]) - np.array([3.0, 17.0, 40.0])).astype(np.float32)
    check(pcm, X, 0.37, rng.integers(0, 5, 4096), 5)
    sup, want = check(pcm, X, 0.37 * 4)                      # the same cloud where most rows have neighbours
    assert sup.cell_log2 == 1 and want.max() >= 4


def test_general_floats_on_the_positive_box(pcm):
    rng = np.random.default_rng(4)
    X = (rng.random((4096, 3)) * np.array([8.0, 64.0, 64.0])).astype(np.float32)
    X[1::2] = X[::2] + np.float32(0.2) * rng.standard_normal((2048, 3)).astype(np.float32)   # pairs around 0.37 apart
    sup, want = check(pcm, X, 0.37)
    assert sup.cell_log2 == -1 and want.max() >= 1


def raster_days(h=37, w=150, seed=8):
    """Three days of one h x w raster surface, each with its own speckle far off the surface."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    clouds, groups = [], []
    for g in range(3):
        z = 3.0 * np.sin(xx / 23.0) + 2.0 * np.cos(yy / 7.0) + 0.2 * rng.standard_normal(xx.shape)
        c = np.stack([z, yy, xx], axis=-1).reshape(-1, 3)[rng.random(h * w) < 0.5]
        k = 20
        speckle = np.stack([rng.uniform(8, 30, k) * rng.choice([-1, 1], k), rng.uniform(0, h, k), rng.uniform(0, w, k)], 1)
        clouds.append(np.concatenate([c, speckle]).astype(np.float32))
        groups.append(np.full(clouds[-1].shape[0], g))
    return clouds, np.concatenate(groups)


def test_raster_days_with_speckle(pcm):
    clouds, groups = raster_days()
    X = np.concatenate(clouds)
    sup, want = check(pcm, X, 1.6, groups, 3)
    days = sup.days.cpu().numpy()
    assert (days == 3).sum() > X.shape[0] // 2 and (want == 0).sum() >= 30      # surface on all days; lone speckle


@pytest.mark.parametrize("r", (0.5, 1.0, 1.25, 3.0))
def test_faces(pcm, r):
    X = S.face_cloud(r)
    near = S.predicate(X, r)
    d = X.astype(np.float64)[:, None, :] - X.astype(np.float64)[None, :, :]
    assert (near & ((d * d).sum(-1) == r * r)).any()          # pairs at exactly r are in the cloud
    sup, _ = check(pcm, X, r, np.arange(X.shape[0]) % 7, 7)
    assert sup.cell_log2 == S.radius_exponent(r)


@pytest.mark.parametrize("extra", (-1, 0, 1, None))
def test_crowded_cells(pcm, extra):
    from pcm_amd import _lib
    chunk = _lib.SUPPORT_CHUNK
    m = 3 * chunk + 5 if extra is None else chunk + extra
    rng = np.random.default_rng(m)
    around = (rng.random((300, 3)) * 4.0 - 2.0).astype(np.float32)
    X = np.concatenate([np.tile(np.float32([0.25, -0.5, 0.125]), (m, 1)), around])
    X = X[rng.permutation(X.shape[0])]
    _, want = check(pcm, X, 1.0)
    top = int(want.max())
    assert top >= m - 1
    for cap in (1, 7, top, top + 1):
        check(pcm, X, 1.0, max_count=cap)
    check(pcm, X, 1.0, np.arange(X.shape[0]) % 4, 4, max_count=7)     # days are exact whatever the cap


def test_sizes(pcm):
    from pcm_amd import _lib
    rng = np.random.default_rng(1)
    tpb = _lib.SUPPORT_TPB
    for n in (0, 1, 2, 63, 64, 65, tpb - 1, tpb, tpb + 1):
        X = (rng.random((n, 3)) * 3.0).astype(np.float32)
        sup, _ = check(pcm, X, 0.8, np.arange(n) % 2, 2)
        assert sup.counts.shape == (n,) and sup.days.shape == (n,)
        check(pcm, X, 0.8)


def test_thin_clouds(pcm):
    rng = np.random.default_rng(6)
    X = (rng.random((1500, 3)) * np.array([0.0, 30.0, 30.0]) + np.array([2.5, 0.0, 0.0])).astype(np.float32)
    check(pcm, X, 0.9)                                                # constant z
    t = rng.random(1500).astype(np.float32) * 40
    check(pcm, np.stack([t * 0.5, -t, t * 0.25], axis=1), 0.1)        # all rows on a line
    check(pcm, np.tile(np.float32([1, 2, 3]), (200, 1)), 0.1)         # one point, 200 times


def test_forced_coarsening(pcm):
    rng = np.random.default_rng(9)
    a = (rng.random((400, 3)) * 0.05).astype(np.float32)
    X = np.concatenate([a, a[::-1] + np.float32([0, 0, 1e6])]).astype(np.float32)
    sup, want = check(pcm, X, 0.01)
    assert S.radius_exponent(0.01) == -6 and sup.cell_log2 == S.plan(X, 0.01)[0] > -6
    assert want[:400].max() >= 1
    far = (rng.random((300, 3)) * 0.05).astype(np.float32) + np.float32(1e30)     # the magnitude rule
    sup, _ = check(pcm, far, 0.01)
    assert sup.cell_log2 == S.plan(far, 0.01)[0] > 40


def test_order_and_groups(pcm):
    rng = np.random.default_rng(12)
    X = (rng.random((2000, 3)) * np.array([2.0, 20.0, 20.0])).astype(np.float32)
    groups = rng.integers(0, 64, 2000)
    groups[:5] = 63
    sup, c0, d0 = run(pcm, X, 1.1, groups, 64)
    want_c, want_d, _ = S.brute(X, 1.1, groups, 64)
    assert np.array_equal(c0, want_c) and np.array_equal(d0, want_d)
    X2 = np.concatenate([X, np.float32([[50, 50, 50], [50, 50, 50.5]])])
    g2 = np.concatenate([groups, [63, 0]])
    _, c2, d2 = run(pcm, X2, 1.1, g2, 64)
    assert d2[-2:].tolist() == [2, 2] and c2[-2:].tolist() == [1, 1]     # group 63 is counted
    perm = rng.permutation(2000)
    _, c1, d1 = run(pcm, X[perm], 1.1, groups[perm], 64)
    assert np.array_equal(c1, c0[perm]) and np.array_equal(d1, d0[perm])
    with pytest.raises(ValueError, match="n_groups must be 1..64"):
        pcm.radius_support(dev(X), 1.1, groups=dev(groups), n_groups=65)
    with pytest.raises(ValueError, match="n_groups must be 1..64"):
        pcm.radius_support(dev(X), 1.1, groups=dev(np.arange(2000) % 65))
    with pytest.raises(ValueError, match="groups must lie"):
        pcm.radius_support(dev(X), 1.1, groups=dev(groups), n_groups=63)
    with pytest.raises(ValueError, match="max_count"):
        pcm.radius_support(dev(X), 1.1, max_count=-2)
    with pytest.raises(ValueError, match="radius"):
        pcm.radius_support(dev(X), 0.0)
    with pytest.raises(ValueError, match="float32"):
        pcm.radius_support(dev(X).double(), 1.0)


def test_nonfinite_rows(pcm):
    rng = np.random.default_rng(13)
    X = (rng.random((1000, 3)) * 6.0).astype(np.float32)
    X[::2] = X[1::2] + np.float32(0.01)                     # every row has a neighbour ...
    bad = rng.choice(1000, 40, replace=False)
    X[bad[:15], 0] = np.nan                                 # ... until its partner is not a point
    X[bad[15:30], 2] = np.inf
    X[bad[30:], 1] = -np.inf
    sup, want = check(pcm, X, 0.5, np.arange(1000) % 3, 3)
    assert sup.skipped == 40 and not sup.counts.cpu().numpy()[bad].any() and not sup.days.cpu().numpy()[bad].any()
    clean = X.copy()
    clean[bad] = 1e6 + np.arange(40, dtype=np.float32)[:, None] * 100
    assert np.array_equal(np.delete(want, bad), np.delete(S.brute(clean, 0.5)[0], bad))
    check(pcm, np.full((70, 3), np.nan, dtype=np.float32), 1.0, np.zeros(70, dtype=np.int64), 1)   # no finite row at all


def test_filter_outliers_mask(pcm):
    clouds, groups = raster_days()
    X = np.concatenate(clouds)
    X[5, 1] = np.nan
    for min_neighbors, min_days in ((1, 1), (4, 1), (3, 2), (0, 3)):
        g = dict(groups=dev(groups), n_groups=3) if min_days > 1 else {}
        keep = pcm.filter_outliers(dev(X), 1.6, min_neighbors, min_days=min_days, **g)
        assert keep.dtype == torch.bool and keep.shape == (X.shape[0],)
        want = S.keep_mask(X, 1.6, min_neighbors, min_days, groups if min_days > 1 else None, 3)
        assert np.array_equal(keep.cpu().numpy(), want) and not want[5]
    assert pcm.filter_outliers(dev(X[:0]), 1.0).shape == (0,)


def test_kmeans_fuse_with_denoise_equals_the_prefiltered_fuse(pcm):
    from pcm_amd import plugin
    clouds, groups = raster_days(20, 60, seed=15)
    X = np.concatenate(clouds)
    want = S.keep_mask(X, 1.6, 3, 2, groups, 3)
    assert 0 < (~want).sum() < X.shape[0] // 4
    c64 = [c.astype(np.float64) for c in clouds]
    _, res = plugin.kmeans_fuse(c64, n_clusters=32, max_iter=10, denoise=(1.6, 3, 2))
    assert np.array_equal(res["denoise"]["kept"], want)
    assert res["denoise"]["removed"] == [int((~want[groups == g]).sum()) for g in range(3)]
    pre = [c[want[groups == g]] for g, c in enumerate(c64)]
    _, ref = plugin.kmeans_fuse(pre, n_clusters=32, max_iter=10)
    assert np.array_equal(res["labels"], ref["labels"]) and np.array_equal(res["centers"], ref["centers"])
    assert res["n_iter"] == ref["n_iter"] and res["inertia"] == ref["inertia"]
    _, one = plugin.kmeans_assign(c64[1:2], res, denoise=(1.6, 3))
    assert np.array_equal(one["denoise"]["kept"], S.keep_mask(clouds[1], 1.6, 3))
