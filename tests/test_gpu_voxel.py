"""GPU: ``voxel_grid`` / ``voxel_downsample`` and the plugin's ``voxel=``, every output bitwise against
the NumPy restatement (tests/voxel_ref.py): whichever waves a voxel's rows fall into and whichever
way the sort orders them, the cells, counts, sums, first rows, day masks and inverse are the same
integers.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import voxel_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu


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


def host(t):
    return None if t is None else t.cpu().numpy()


def run(pcm, X, voxel, origin=(0.0, 0.0, 0.0), groups=None, n_groups=None, q=None):
    vox = pcm.voxel_grid(dev(X, np.float32), voxel, origin=origin, groups=None if groups is None else dev(groups),
                         n_groups=n_groups, q=q)
    torch.cuda.synchronize()
    return vox


def check(pcm, X, voxel, origin=(0.0, 0.0, 0.0), groups=None, n_groups=None, q=None):
    """The kernels against the reference, every array bitwise; -> (Voxels, the reference dict)."""
    ref = V.voxel_grid(X, voxel, origin, groups, q)
    vox = run(pcm, X, voxel, origin, groups, n_groups, q)
    M = ref["cells"].shape[0]
    assert vox.cells.shape == (M, 3) and vox.skipped == ref["skipped"] and vox.q == ref["q"]
    for name, dtype in (("cells", np.int64), ("counts", np.int32), ("sums", np.int64), ("first", np.int32),
                        ("inverse", np.int32)):
        got = host(getattr(vox, name))
        assert got.dtype == dtype and got.shape == ref[name].shape and np.array_equal(got, ref[name]), name
    if groups is None:
        assert vox.day_mask is None
    else:
        got = host(vox.day_mask)
        assert got.dtype == np.int64 and np.array_equal(got, ref["day_mask"])
        assert np.array_equal(host(vox.days()), V.days(ref))
    assert np.array_equal(np.float32(vox.inv), ref["inv"])
    return vox, ref


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65))
def test_small_n(pcm, n):
    rng = np.random.default_rng(n)
    X = (rng.random((n, 3)) * 3.0 - 1.0).astype(np.float32)
    vox, _ = check(pcm, X, 1.0)
    assert vox.inverse.shape == (n,) and vox.day_mask is None
    check(pcm, X, 1.0, groups=np.arange(n) % 2, n_groups=2)
    check(pcm, X, 8.0, groups=np.arange(n) % 3, n_groups=3)          # all rows in few voxels


def test_all_in_one_voxel(pcm):
    rng = np.random.default_rng(1)
    X = (rng.random((1000, 3)) * 0.9 + np.array([2.0, -3.0, 0.05])).astype(np.float32)
    vox, ref = check(pcm, X, 1.0, groups=rng.integers(0, 7, 1000), n_groups=7)
    assert ref["cells"].tolist() == [[2, -3, 0]] and ref["counts"].tolist() == [1000] and ref["first"].tolist() == [0]


def test_one_voxel_per_row(pcm):
    n = 64 * 257 + 1
    rng = np.random.default_rng(2)
    i = rng.permutation(n)
    X = np.stack([(i // 4096).astype(np.float32), ((i // 64) % 64).astype(np.float32), (i % 64).astype(np.float32)], 1)
    vox, ref = check(pcm, X + np.float32(0.5), 1.0, groups=i % 64, n_groups=64)
    assert ref["cells"].shape[0] == n and (ref["counts"] == 1).all()


def test_more_than_one_scan_tile(pcm):
    """The heads are scanned in tiles of 1024 waves (65536 sorted rows): three tiles, the last partial."""
    n = 2 * 65536 + 77
    rng = np.random.default_rng(3)
    X = (rng.random((n, 3)) * np.array([4.0, 100.0, 100.0])).astype(np.float32)
    X[::1000, 2] = np.nan
    vox, ref = check(pcm, X, 1.0, groups=rng.integers(0, 4, n), n_groups=4)
    end = np.cumsum(ref["counts"])
    assert ref["cells"].shape[0] > 30000 and ((end - ref["counts"]) // 65536 != (end - 1) // 65536).any()   # a segment across tiles


def test_voxel_populations_around_the_wave_and_block_edges(pcm):
    X, pops = V.edge_cloud()
    groups = np.arange(X.shape[0]) % 5
    vox, ref = check(pcm, X, (1.0, 1.0, 1.0), groups=groups, n_groups=5)
    assert ref["counts"].tolist() == pops
    for want in (63, 64, 65, 127, 128, 129, 255, 256, 257, 3 * 256 + 5):
        assert want in pops
    # the sorted layout is the voxel order: where the segments begin and end
    end = np.cumsum(ref["counts"])
    beg = end - ref["counts"]
    spans_waves = (beg // 64) != ((end - 1) // 64)
    assert (beg % 64 == 0).any() and (end % 64 == 0).any() and (beg % 256 == 0).any() and (end % 256 == 0).any()
    assert (spans_waves & (beg % 64 != 0) & (end % 64 != 0)).any()              # begins and ends inside waves, spans one
    assert (((end - 1) // 64 - beg // 64) >= 2).any()                            # whole waves inside one segment
    assert ((beg // 256) != ((end - 1) // 256)).any()                            # spans a block boundary
    assert (~spans_waves & (ref["counts"] > 1)).any() and (ref["counts"] == 1).any()
    # a segment that is exactly one wave, and waves holding three or more segments
    assert ((beg % 64 == 0) & (ref["counts"] == 64)).any()
    assert np.bincount(beg // 64).max() >= 3
    # the duplicates: one centroid equal to the point itself
    j = pops.index(3 * 256 + 5)
    assert np.array_equal(host(vox.centroids())[j], X[ref["first"][j]])


@pytest.mark.parametrize("voxel", (0.5, 0.3, (0.25, 1.0, 1.0)))
def test_sizes_faces_origin_and_negative_zero(pcm, voxel):
    X = V.face_cloud()
    assert (X < 0).any() and (np.signbit(X) & (X == 0)).any()
    v, inv = V.sizes(voxel)
    on_face = (np.floor(X * inv) == X * inv).any(axis=1)
    assert on_face.sum() > 100
    vox, ref = check(pcm, X, voxel)
    assert (ref["cells"] < 0).any() and ref["counts"].max() >= 2
    vox2, ref2 = check(pcm, X, voxel, origin=(0.125, -1.5, 0.3), groups=np.arange(X.shape[0]) % 5, n_groups=5)
    assert vox2.origin == (0.125, -1.5, float(np.float32(0.3))) and vox2.voxel == tuple(float(t) for t in v)
    assert not np.array_equal(ref["cells"], ref2["cells"])
    check(pcm, X, voxel, q=[t - 3 for t in ref["q"]])                  # an explicit q
    with pytest.raises(ValueError, match="q must hold 3"):
        pcm.voxel_grid(dev(X), voxel, q=[20, 20])


def test_nonfinite_rows(pcm):
    rng = np.random.default_rng(13)
    X = (rng.random((3000, 3)) * 6.0 - 2.0).astype(np.float32)
    bad = rng.choice(3000, 90, replace=False)
    X[bad[:30], 0] = np.nan
    X[bad[30:60], 2] = np.inf
    X[bad[60:], 1] = -np.inf
    X[bad[:5]] = np.nan
    vox, ref = check(pcm, X, 0.5, groups=np.arange(3000) % 3, n_groups=3)
    assert vox.skipped == 90 and (host(vox.inverse)[bad] == -1).all() and (np.delete(host(vox.inverse), bad) >= 0).all()
    # q comes from the finite rows alone
    X[bad[0]] = [np.nan, 1e6, 1e6]
    assert check(pcm, X, 0.5)[0].q == ref["q"]
    vox, ref = check(pcm, np.full((70, 3), np.nan, dtype=np.float32), 1.0, groups=np.zeros(70, dtype=np.int64), n_groups=1)
    assert vox.cells.shape == (0, 3) and vox.skipped == 70 and vox.day_mask.shape == (0,) and vox.centroids().shape == (0, 3)


@pytest.mark.parametrize("G", (1, 5, 64))
def test_groups(pcm, G):
    rng = np.random.default_rng(G)
    X = (rng.random((5000, 3)) * np.array([2.0, 12.0, 12.0])).astype(np.float32)
    groups = rng.integers(0, G, 5000)
    groups[:40] = G - 1
    vox, ref = check(pcm, X, 1.0, groups=groups, n_groups=G)
    if G == 64:
        assert (ref["day_mask"] < 0).any()                             # bit 63 is the sign bit
        assert check(pcm, X, 1.0, groups=groups.astype(np.uint8))[0].day_mask is not None       # n_groups from the maximum
    assert run(pcm, X, 1.0).day_mask is None
    with pytest.raises(ValueError, match="n_groups must be 1..64"):
        pcm.voxel_grid(dev(X), 1.0, groups=dev(groups), n_groups=65)
    with pytest.raises(ValueError, match="groups must lie"):
        pcm.voxel_grid(dev(X), 1.0, groups=dev(groups + 1), n_groups=G)
    with pytest.raises(ValueError, match="groups must be"):
        pcm.voxel_grid(dev(X), 1.0, groups=dev(groups[:-1]))
    with pytest.raises(ValueError, match="float32"):
        pcm.voxel_grid(dev(X).double(), 1.0)


def test_row_order_invariance(pcm):
    X = V.face_cloud(2500, seed=7)
    X[::97, 1] = np.nan
    groups = np.arange(X.shape[0]) % 6
    a = run(pcm, X, 0.3, (0.1, 0.2, 0.3), groups, 6)
    perm = np.random.default_rng(8).permutation(X.shape[0])
    b = run(pcm, X[perm], 0.3, (0.1, 0.2, 0.3), groups[perm], 6)
    for name in ("cells", "counts", "sums", "day_mask"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.skipped == b.skipped and a.q == b.q
    ia, ib, fa, fb = host(a.inverse), host(b.inverse), host(a.first), host(b.first)
    assert np.array_equal(ib, ia[perm])                                 # the same voxel for the same point
    pos = np.empty_like(perm)
    pos[perm] = np.arange(perm.size)                                    # old row -> new row
    for j in range(0, fa.size, 37):                                     # first: the lowest NEW row of the same voxel
        assert fb[j] == pos[np.flatnonzero(ia == j)].min()
    assert (ib[fb] == np.arange(fb.size)).all() and (ia[fa] == np.arange(fa.size)).all()


def test_cluster_stats_cross_check(pcm):
    rng = np.random.default_rng(21)
    X = (rng.random((6000, 3)) * np.array([1.5, 9.0, 9.0]) - np.array([0.5, 2.0, 3.0])).astype(np.float32)
    vox = run(pcm, X, (0.5, 1.0, 1.0))
    M = vox.cells.shape[0]
    assert 100 < M <= 1024 and vox.skipped == 0
    st = pcm.cluster_stats(dev(X), vox.inverse, M, q=vox.q)
    assert np.array_equal(st.counts()[0], host(vox.counts)) and np.array_equal(st.sums()[0], host(vox.sums))
    assert np.array_equal(st.means()[0].astype(np.float32), host(vox.centroids()))


def test_voxel_downsample(pcm):
    X = V.face_cloud(3000, seed=9)
    X[5] = np.nan
    groups = np.arange(X.shape[0]) % 4
    ref = V.voxel_grid(X, 0.5)
    ds = pcm.voxel_downsample(dev(X), 0.5)
    assert ds.points.dtype == torch.float32 and ds.points.is_cuda and ds.rows.dtype == torch.int32
    assert np.array_equal(host(ds.points), V.centroids(ref)) and np.array_equal(host(ds.rows), ref["first"])
    assert np.array_equal(host(ds.voxels.centroids()), V.centroids(ref)) and host(ds.kept).all()
    ds = pcm.voxel_downsample(dev(X), 0.5, mode="first")
    assert np.array_equal(host(ds.points), X[ref["first"]]) and np.array_equal(host(ds.rows), ref["first"])
    for mode in ("centroid", "first"):
        for min_count, min_days in ((2, 1), (1, 2), (3, 3)):
            want_p, want_r, r = V.downsample(X, 0.5, mode, (0.25, 0, 0), min_count, min_days, groups)
            ds = pcm.voxel_downsample(dev(X), 0.5, mode=mode, origin=(0.25, 0, 0), min_count=min_count, min_days=min_days,
                                      groups=dev(groups), n_groups=4)
            assert 0 < want_r.size < r["counts"].size
            assert np.array_equal(host(ds.points), want_p) and np.array_equal(host(ds.rows), want_r)
            assert int(ds.kept.sum()) == want_r.size and ds.voxels.cells.shape[0] == r["counts"].size
    empty = pcm.voxel_downsample(dev(X[:0]), 0.5)
    assert empty.points.shape == (0, 3) and empty.rows.shape == (0,)


def raster_days(h=30, w=80, seed=15):
    """Three days of one h x w surface sampled at half-pixel spacing, each day its own subset."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(0, h, 0.5), np.arange(0, w, 0.5), indexing="ij")
    clouds = []
    for g in range(3):
        z = 3.0 * np.sin(xx / 23.0) + 2.0 * np.cos(yy / 7.0) + 0.1 * rng.standard_normal(xx.shape)
        clouds.append(np.stack([z, yy, xx], axis=-1).reshape(-1, 3)[rng.random(xx.size) < 0.4 + 0.2 * g])
    return clouds


def test_kmeans_fuse_with_voxel_equals_the_fuse_of_the_thinned_clouds(pcm):
    from pcm_amd import plugin
    clouds = raster_days()
    size = (0.5, 1.0, 1.0)
    parts = [V.thin(c.astype(np.float32), size) for c in clouds]
    _, res = plugin.kmeans_fuse(clouds, n_clusters=32, max_iter=10, voxel=size)
    vox = res["voxel"]
    assert vox["size"] == size and vox["kept_rows"] == [p[0].shape[0] for p in parts]
    assert all(k < c.shape[0] for k, c in zip(vox["kept_rows"], clouds))
    assert np.array_equal(vox["counts"], np.concatenate([p[1] for p in parts]))
    off = np.cumsum([0] + vox["kept_rows"][:-1])
    assert np.array_equal(vox["inverse"], np.concatenate([p[2] + o for p, o in zip(parts, off)]))
    _, ref = plugin.kmeans_fuse([p[0].astype(np.float64) for p in parts], n_clusters=32, max_iter=10)
    assert np.array_equal(res["labels"], ref["labels"]) and np.array_equal(res["centers"], ref["centers"])
    assert res["n_iter"] == ref["n_iter"] and res["inertia"] == ref["inertia"] and res["n_points"] == sum(vox["kept_rows"])
    assert res["labels"][vox["inverse"]].shape == (sum(c.shape[0] for c in clouds),)


def test_value_errors_from_the_device(pcm):
    far = np.array([[0, 0, 0], [0, 0, 1e7]], dtype=np.float32)
    with pytest.raises(ValueError, match="voxel.*2\\^21"):
        pcm.voxel_grid(dev(far), 1.0)
    check(pcm, far, 8.0)
    with pytest.raises(ValueError, match="voxel.*2\\^40"):
        pcm.voxel_grid(dev(np.full((2, 3), 1e30, dtype=np.float32)), 0.01)
    with pytest.raises(ValueError, match="voxel.*not finite"):
        pcm.voxel_grid(dev(np.full((2, 3), 3e38, dtype=np.float32)), 1e-3)
    with pytest.raises(ValueError, match="voxel.*not finite"):
        pcm.voxel_grid(dev(np.full((2, 3), 3e38, dtype=np.float32)), 1.0, origin=(-3e38, 0, 0))
    edge = np.array([[0, 0, 0], [np.nan, 0, 0], [0, 0, 2 ** 21 - 1]], dtype=np.float32)
    check(pcm, edge, 1.0)                                               # exactly 2^21 cells on an axis
    edge[2, 2] = 2 ** 21
    with pytest.raises(ValueError, match="voxel"):
        pcm.voxel_grid(dev(edge), 1.0)
    with pytest.raises(ValueError, match="voxel"):
        pcm.voxel_downsample(dev(far), 1.0)
