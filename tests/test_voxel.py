"""CPU: the voxel reference (tests/voxel_ref.py) pinned to ``np.unique`` on an exact lattice and to a
hand case, the argument checks of the four entry points and of the Python layer, and the plugin's
``voxel=`` path through the ``voxels=`` stand-in (the product has no CPU fallback; the HIP kernels
are checked in tests/test_gpu_voxel.py).
"""
import ctypes
import os

import numpy as np
import pytest

import voxel_ref as V
from oracle import lloyd_ref as R


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("v", (0.5, 1.0, 2.0, (0.25, 1.0, 2.0)))
def test_reference_equals_unique_on_the_lattice(v):
    """Power-of-two sizes: the float32 cell rule is exact, so float64 floor(X / v) must agree; the
    lattice has points exactly on the faces and negative coordinates, so floor (not trunc) is pinned."""
    X = V.lattice_cloud()
    ref = V.voxel_grid(X, v)
    vv = np.broadcast_to(np.asarray(v, dtype=np.float64), (3,))
    c64 = np.floor(X.astype(np.float64) / vv)
    cells, inverse, counts = np.unique(c64, axis=0, return_inverse=True, return_counts=True)
    assert np.array_equal(ref["cells"], cells.astype(np.int64))
    assert np.array_equal(ref["inverse"], inverse.reshape(-1)) and np.array_equal(ref["counts"], counts)
    on_face = (X.astype(np.float64) / vv == c64).any(axis=1)
    assert on_face.sum() > 100 and (c64 < 0).any() and (np.trunc(X / vv) != c64).any()
    # sums and first against a per-voxel loop
    q = np.asarray(ref["q"])
    for j in (0, len(counts) // 2, len(counts) - 1):
        rows = np.flatnonzero(inverse.reshape(-1) == j)
        assert ref["first"][j] == rows.min()
        assert np.array_equal(ref["sums"][j], np.trunc(np.ldexp(X[rows].astype(np.float64), q)).astype(np.int64).sum(0))
    assert ref["skipped"] == 0 and ref["day_mask"] is None


def test_reference_on_a_hand_case():
    X = np.array([[1.5, 10.0, -3.0],      # cell (0, 0, -1) at origin (1, 10, -2.5), voxel 1
                  [1.5, 10.0, -3.0],      # its duplicate
                  [np.nan, 0, 0],
                  [0.99, 10.0, -2.5],     # cell (-1, 0, 0): just below the origin on z, on the face on x
                  [1.0, 10.5, -2.5],      # cell (0, 0, 0): exactly on the origin
                  [0, np.inf, 0],
                  [1.25, 10.75, -2.0]],   # cell (0, 0, 0)
                 dtype=np.float32)
    groups = [63, 0, 5, 2, 63, 5, 1]
    ref = V.voxel_grid(X, 1.0, origin=(1.0, 10.0, -2.5), groups=groups)
    assert ref["cells"].tolist() == [[-1, 0, 0], [0, 0, -1], [0, 0, 0]]
    assert ref["counts"].tolist() == [1, 2, 2] and ref["first"].tolist() == [3, 0, 4]
    assert ref["inverse"].tolist() == [1, 1, -1, 0, 2, -1, 2] and ref["skipped"] == 2
    assert ref["day_mask"].dtype == np.int64
    assert ref["day_mask"].tolist() == [1 << 2, (1 << 0) - (1 << 63), (1 << 1) - (1 << 63)]     # group 63: the sign bit
    assert V.days(ref).tolist() == [1, 2, 2]
    assert ref["q"] == [24, 21, 23]                                        # max |x| = 1.5, 10.75, 3 over the finite rows
    assert ref["sums"][1].tolist() == [3 << 24, 20 << 21, -(6 << 23)]
    assert np.array_equal(V.centroids(ref), np.float32([[0.99, 10, -2.5], [1.5, 10, -3], [1.125, 10.625, -2.25]]))
    pts, rows, _ = V.downsample(X, 1.0, "first", (1.0, 10.0, -2.5), min_count=2)
    assert rows.tolist() == [0, 4] and np.array_equal(pts, X[[0, 4]])
    pts, rows, _ = V.downsample(X, 1.0, "centroid", (1.0, 10.0, -2.5), min_days=2, groups=groups)
    assert rows.tolist() == [0, 4]
    none = V.voxel_grid(X[[2, 5]], 1.0, groups=[0, 1])
    assert none["cells"].shape == (0, 3) and none["skipped"] == 2 and none["inverse"].tolist() == [-1, -1]
    assert none["day_mask"].shape == (0,) and none["q"] == [25, 25, 25]


def test_inverse_is_rounded_for_other_sizes():
    v, inv = V.sizes(0.3)
    assert inv[0] == np.float32(1.0 / np.float64(np.float32(0.3))) and inv.dtype == np.float32
    # 1.5f * inv rounds to 5.0 in float32 although 1.5 / 0.3f < 5 in exact arithmetic: the rule is the definition
    x = np.float32(1.5)
    assert float(x) / float(v[0]) < 5.0 and V.cellf(x, 0.0, inv[0]) == 5.0


def test_span_and_magnitude_rules_raise():
    far = np.array([[0, 0, 0], [0, 0, 1e7]], dtype=np.float32)
    with pytest.raises(ValueError, match="voxel.*2\\^21"):
        V.voxel_grid(far, 1.0)
    assert V.voxel_grid(far, 8.0)["cells"].tolist() == [[0, 0, 0], [0, 0, 1250000]]
    with pytest.raises(ValueError, match="voxel.*2\\^40"):
        V.voxel_grid(np.full((2, 3), 1e30, dtype=np.float32), 0.01)
    with pytest.raises(ValueError, match="voxel.*not finite"):
        V.voxel_grid(np.full((2, 3), 3e38, dtype=np.float32), 1e-3)
    with pytest.raises(ValueError, match="voxel.*not finite"):
        V.voxel_grid(np.full((2, 3), 3e38, dtype=np.float32), 1.0, origin=(-3e38, 0, 0))     # x - o overflows
    # exactly 2^21 cells on one axis is allowed, one more is not
    edge = np.array([[0, 0, 0], [0, 0, 2 ** 21 - 1]], dtype=np.float32)
    assert V.voxel_grid(edge, 1.0)["cells"][-1].tolist() == [0, 0, 2 ** 21 - 1]
    edge[1, 2] = 2 ** 21
    with pytest.raises(ValueError, match="voxel"):
        V.voxel_grid(edge, 1.0)


# ---------------------------------------------------------------- the C ABI without a device
@pytest.fixture(scope="module")
def lib():
    from pcm_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.load(require_gpu_runtime=False)


def f3(*v):
    return (ctypes.c_float * 3)(*v)


def test_voxel_argument_errors_without_device(lib):
    from pcm_amd import _lib
    nbytes = ctypes.c_size_t()
    assert lib.pcm_voxel_workspace(-1, ctypes.byref(nbytes)) == -1
    assert "pcm_voxel_workspace" in _lib.last_error()
    assert lib.pcm_voxel_workspace(1 << 31, ctypes.byref(nbytes)) == -1
    assert lib.pcm_voxel_workspace(10, None) == -1
    assert lib.pcm_voxel_workspace(6400, ctypes.byref(nbytes)) == 0 and nbytes.value >= 100 * 4
    one, zero = f3(1, 1, 1), f3(0, 0, 0)
    assert lib.pcm_voxel_keys(None, -1, one, zero, None, None, None) == -1
    assert "pcm_voxel_keys" in _lib.last_error() and "n must be" in _lib.last_error()
    assert lib.pcm_voxel_keys(None, 1 << 31, one, zero, None, None, None) == -1
    assert lib.pcm_voxel_keys(None, 5, None, zero, None, None, None) == -1
    for bad in (f3(0, 1, 1), f3(1, -1, 1), f3(1, 1, float("nan")), f3(float("inf"), 1, 1), f3(1, 1e-45, 1), f3(1, 1, 3e38)):
        assert lib.pcm_voxel_keys(None, 5, bad, zero, None, None, None) == -1
        assert "voxel sizes" in _lib.last_error()
    assert lib.pcm_voxel_keys(None, 5, one, f3(0, float("inf"), 0), None, None, None) == -1
    assert "origin" in _lib.last_error()
    assert lib.pcm_voxel_keys(None, 5, one, zero, None, None, None) == -1           # no info block
    assert "info is null" in _lib.last_error()
    assert lib.pcm_voxel_count(None, -1, None, None, 0, None) == -1
    assert "pcm_voxel_count" in _lib.last_error()
    assert lib.pcm_voxel_count(None, 1 << 31, None, None, 0, None) == -1
    assert lib.pcm_voxel_count(None, 5, None, None, 0, None) == -1                    # null pointers
    assert lib.pcm_voxel_count(None, 0, None, None, 0, None) == 0                     # nothing to count
    q = (ctypes.c_int32 * 3)(25, 25, 25)
    rest = (None,) * 7 + (None, 0, None)
    assert lib.pcm_voxel_reduce(None, -1, None, 1, q, None, None, 0, *rest) == -1
    assert "pcm_voxel_reduce" in _lib.last_error()
    assert lib.pcm_voxel_reduce(None, 1 << 31, None, 1, q, None, None, 0, *rest) == -1
    assert lib.pcm_voxel_reduce(None, 5, None, 1, q, None, None, 6, *rest) == -1
    assert "m must be" in _lib.last_error()
    for g in (0, 65):
        assert lib.pcm_voxel_reduce(None, 5, None, g, q, None, None, 0, *rest) == -1
        assert "n_groups must be 1..64" in _lib.last_error()
    assert lib.pcm_voxel_reduce(None, 5, None, 1, q, None, None, 0, *rest) == -1      # null pointers
    assert "is null" in _lib.last_error()
    assert lib.pcm_voxel_reduce(None, 0, None, 1, q, None, None, 0, *rest) == 0       # nothing to reduce


def test_constants_mirror_the_header():
    import re
    from pcm_amd import _lib
    src = open(os.path.join(_lib.REPO_DIR, "include", "pcm_kmeans.h")).read()
    for name, value in (("TPB", _lib.VOXEL_TPB), ("MAXG", _lib.VOXEL_MAXG), ("INFO_WORDS", _lib.VOXEL_INFO_WORDS),
                        ("E_NONFINITE", _lib.VOXEL_E_NONFINITE), ("E_MAGNITUDE", _lib.VOXEL_E_MAGNITUDE),
                        ("E_SPAN", _lib.VOXEL_E_SPAN)):
        assert int(re.search(rf"#define PCM_VOXEL_{name} (\d+)", src).group(1)) == value
    assert _lib.VOXEL_TPB % 64 == 0 and _lib.ABI_VERSION == 8
    assert int(re.search(r"#define PCM_ABI_VERSION (\d+)", src).group(1)) == 8


# ---------------------------------------------------------------- the Python layer
def test_python_validation_without_device():
    torch = pytest.importorskip("torch")
    import pcm_amd
    from pcm_amd import _lib, voxel
    assert {"voxel_grid", "voxel_downsample", "Voxels", "Downsampled"} <= set(pcm_amd.__all__)
    assert "voxel_grid(" in pcm_amd.__doc__ and "voxel_downsample(" in pcm_amd.__doc__
    X = torch.zeros(4, 3)
    for fn in (pcm_amd.voxel_grid, pcm_amd.voxel_downsample):
        with pytest.raises(_lib.PcmError, match="no CPU fallback"):
            fn(X, 1.0)
    for bad in (0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, "x", (1, 2), (1, 2, 0), None, 1e-45, 3e38):
        with pytest.raises(ValueError, match="voxel"):
            voxel.voxel_sizes(bad)
    v, inv = voxel.voxel_sizes(0.3)
    want_v, want_inv = V.sizes(0.3)
    assert np.array_equal(v, want_v) and np.array_equal(inv, want_inv) and inv.dtype == np.float32
    assert voxel.voxel_sizes((0.25, 1, 2))[0].tolist() == [0.25, 1.0, 2.0]
    for bad in ((0, 0), (0, 0, float("nan")), (0, float("inf"), 0), 1.0, "abc", (1e39, 0, 0)):
        with pytest.raises(ValueError, match="origin"):
            voxel._origin32(bad)
    with pytest.raises(ValueError, match="mode"):
        pcm_amd.voxel_downsample(X, 1.0, mode="median")
    with pytest.raises(ValueError, match="min_count"):
        pcm_amd.voxel_downsample(X, 1.0, min_count=0)
    with pytest.raises(ValueError, match="min_days"):
        pcm_amd.voxel_downsample(X, 1.0, min_days=0)
    with pytest.raises(ValueError, match="needs groups"):
        pcm_amd.voxel_downsample(X, 1.0, min_days=2)
    # the box as the kernel encodes it decodes to the floats
    f = np.float32([-2.5, 0.0, 3e38, -0.0, 1e-40, -1e30])
    b = f.view(np.uint32)
    enc = np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.int64)
    assert np.array_equal(voxel._decode_box(enc).view(np.uint32), b)
    m = torch.tensor([0, 1, -1, -(1 << 63), (1 << 63) - 1, 0x5555555555555555], dtype=torch.int64)
    assert voxel._popcount64(m).tolist() == [0, 1, 64, 1, 63, 32]


# ---------------------------------------------------------------- the plugin
def stub_fit(X, C0, max_iter, tol_abs):
    f = R.lloyd_fit(np.asarray(X, dtype=np.float32), C0, max_iter=max_iter, tol=tol_abs)
    return f["labels"], f["centers"], f["inertia"], f["n_iter"]


def same_layers(a, b):
    assert len(a) == len(b)
    for (da, pa, ka), (db, pb, kb) in zip(a, b):
        assert ka == kb and pa["name"] == pb["name"] and np.array_equal(da, db, equal_nan=True)
        assert set(pa) == set(pb)
        for key, va in pa.get("properties", {}).items():
            assert np.array_equal(va, pb["properties"][key], equal_nan=True), key


def three_days(seed=2):
    """Three days of one gentle surface on a shared 20 x 20 raster at half-pixel spacing: about four
    rows per voxel of (1, 1, 1); day 1 is denser than the others."""
    rng = np.random.default_rng(seed)
    clouds = []
    for g, m in enumerate((900, 1500, 700)):
        yy, xx = rng.integers(0, 40, m) / 2.0, rng.integers(0, 40, m) / 2.0
        z = 0.1 * np.sin(xx / 3.0) + 0.05 * g
        clouds.append(np.stack([z, yy, xx], axis=1))
    return clouds


def test_plugin_without_voxel_is_unchanged():
    from pcm_amd import plugin
    clouds = three_days()

    def forbidden(*a):
        raise AssertionError("voxel=None must not thin")

    l0, r0 = plugin.kmeans_fuse(clouds, n_clusters=16, max_iter=8, fit=stub_fit)
    l1, r1 = plugin.kmeans_fuse(clouds, n_clusters=16, max_iter=8, fit=stub_fit, voxel=None, voxels=forbidden)
    same_layers(l0, l1)
    assert set(r0) == set(r1) and "voxel" not in r1
    for key in r0:
        assert np.array_equal(r0[key], r1[key]), key


def test_plugin_fuse_with_voxel():
    from pcm_amd import plugin
    clouds = three_days()
    seen = []

    def spy(X_, size):
        seen.append((X_.copy(), size))
        return V.thin(X_, size)

    layers, res = plugin.kmeans_fuse(clouds, n_clusters=16, max_iter=8, fit=stub_fit, voxel=(0.5, 1, 1), voxels=spy)
    assert len(seen) == 3 and all(s[1] == (0.5, 1.0, 1.0) for s in seen)              # every cloud separately
    for c, s in zip(clouds, seen):
        assert s[0].dtype == np.float32 and np.array_equal(s[0], c.astype(np.float32))
    parts = [V.thin(c.astype(np.float32), (0.5, 1, 1)) for c in clouds]
    vox = res["voxel"]
    assert vox["size"] == (0.5, 1.0, 1.0) and vox["kept_rows"] == [p[0].shape[0] for p in parts]
    assert all(k < c.shape[0] for k, c in zip(vox["kept_rows"], clouds))               # it thinned
    assert np.array_equal(vox["counts"], np.concatenate([p[1] for p in parts]))
    thin = np.concatenate([p[0] for p in parts])
    assert res["n_points"] == thin.shape[0] == sum(vox["kept_rows"]) and res["labels"].shape == (thin.shape[0],)
    assert np.array_equal(layers[1][0], thin.astype(np.float64))
    # the same as fusing the pre-thinned clouds
    l2, r2 = plugin.kmeans_fuse([p[0] for p in parts], n_clusters=16, max_iter=8, fit=stub_fit)
    same_layers(layers, l2)
    for key in r2:
        assert np.array_equal(res[key], r2[key]), key
    # labels[inverse] labels the original points: a point gets the label of its own voxel's centroid
    inv = vox["inverse"]
    n_in = sum(c.shape[0] for c in clouds)
    assert inv.shape == (n_in,) and inv.min() >= 0 and inv.max() == thin.shape[0] - 1
    at, off = 0, 0
    for c, p in zip(clouds, parts):
        assert np.array_equal(inv[at:at + c.shape[0]], p[2] + off)
        at, off = at + c.shape[0], off + p[0].shape[0]
    lab = res["labels"][inv]
    X = np.concatenate(clouds).astype(np.float32)
    assert lab.shape == (n_in,) and (np.abs(X - thin[inv]) <= np.float32([0.5, 1.0, 1.0])).all()
    assert np.array_equal(np.bincount(inv, minlength=thin.shape[0]), vox["counts"])


def test_plugin_voxel_feeds_describe_and_height_map_the_thinned_rows():
    from pcm_amd import plugin
    clouds = three_days()
    clouds[0] = np.concatenate([clouds[0], [[np.nan, 1.0, 1.0]]])                      # a row of no voxel
    got = {}

    def stats(X_, labels, groups, k, G):
        got["stats"] = (X_.shape[0], labels.shape[0], groups.shape[0], G)
        return np.zeros((G, k, 16), dtype=np.int64)

    def grid(X_, labels, groups, k, G, shape, cell_log2, q):
        got["grid"] = (X_.shape[0], labels.shape[0], groups.shape[0], G)
        return np.zeros((G, 4) + tuple(shape), dtype=np.int64), 0

    _, res = plugin.kmeans_fuse(clouds, n_clusters=8, max_iter=4, fit=stub_fit, voxel=1.0, voxels=V.thin,
                                describe=True, stats=stats, height_map=True, grid=grid)
    kept = res["voxel"]["kept_rows"]
    assert got["stats"] == (sum(kept), sum(kept), sum(kept), 3) == got["grid"]
    assert res["stats"]["sizes"] == res["height_map"]["sizes"] == kept
    assert res["voxel"]["size"] == (1.0, 1.0, 1.0) and res["voxel"]["inverse"][900] == -1
    assert (np.delete(res["voxel"]["inverse"], 900) >= 0).all()


def test_plugin_voxel_after_denoise_and_errors():
    from pcm_amd import plugin
    clouds = three_days()
    order = []

    def support(X_, groups, G, radius, min_neighbors, min_days):
        order.append("denoise")
        keep = np.ones(X_.shape[0], dtype=bool)
        keep[:10] = False
        return keep

    def thin(X_, size):
        order.append("voxel")
        return V.thin(X_, size)

    _, res = plugin.kmeans_fuse(clouds, n_clusters=8, max_iter=4, fit=stub_fit, denoise=(1.5, 1), support=support,
                                voxel=1.0, voxels=thin)
    assert order == ["denoise", "voxel", "voxel", "voxel"]
    assert res["voxel"]["inverse"].shape == (sum(c.shape[0] for c in clouds) - 10,)      # the rows that entered the thinning

    def never(*a):
        raise AssertionError("a bad voxel= must fail before anything is fitted")

    for bad in (0, -1.0, (1, 2), (1, 1, float("nan")), "x", float("inf")):
        with pytest.raises(ValueError, match="voxel"):
            plugin.kmeans_fuse(clouds, n_clusters=8, fit=never, voxel=bad, voxels=never)
    with pytest.raises(ValueError, match="voxels must return"):
        plugin.kmeans_fuse(clouds, n_clusters=8, fit=never, voxel=1.0, voxels=lambda X_, s: (X_, np.ones(3), np.zeros(2)))

    class Base:
        def run(self, kml_path, **kw):
            return [(c, {"name": f"pair {i} {plugin.CLOUD_LAYER_SUFFIX}"}, "points") for i, c in enumerate(clouds)]

    ex = plugin.HeightMapExtractor(base=Base(), n_clusters=8, max_iter=4, fit=stub_fit, voxel=(0.5, 1, 1), voxels=V.thin)
    out = ex.run("x.kml")
    assert len(out) == 5 and ex.last_result["voxel"]["size"] == (0.5, 1.0, 1.0)
    out = plugin.HeightMapExtractor(base=Base(), n_clusters=8, max_iter=4, fit=stub_fit, voxel=-2.0, voxels=V.thin).run("x.kml")
    assert len(out) == 1 and out[0][1]["name"].startswith("Error:") and "voxel" in out[0][1]["name"]
