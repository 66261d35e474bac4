"""CPU: ``pcm_height_grid``'s argument checks, the ``HeightGrid`` accessors on words
from the NumPy reference encoder (tests/grid_ref.py), and the plugin's
``height_map=True`` layers through the ``grid=`` stand-in (the product has no CPU
fallback; the HIP kernel is checked in tests/test_gpu_grid.py).
"""
import ctypes
import os

import numpy as np
import pytest

import grid_ref as GR
from oracle import lloyd_ref as R

PREFIX = "[Multi-day 3D Point Cloud] "
NAMES = ["Fused Height Map", "Fused Height Spread", "Fused Coverage", "Fused Surface Height", "Fused Surface Elements"]


# ---------------------------------------------------------------- ABI
def test_height_grid_argument_errors_without_device():
    """Every argument check runs before any device call; n = 0 makes none."""
    from pcm_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    lib = _lib.load(require_gpu_runtime=False)
    one = ctypes.c_void_p(256)      # a non-null address that is never dereferenced

    def call(X=one, n=10, labels=None, k=1, groups=None, G=1, H=4, W=4, s=0, q=0, out=one):
        return lib.pcm_height_grid(X, n, labels, k, groups, G, H, W, 0.0, 0.0, s, q, out, None)

    for kw, word in ((dict(H=0), "H and W"), (dict(W=0), "H and W"), (dict(H=(1 << 24) + 1), "H and W"),
                     (dict(G=2, H=1 << 15, W=1 << 15), "2^31"), (dict(G=0), "n_groups"), (dict(G=257), "n_groups"),
                     (dict(k=0), "k must be"), (dict(n=-1), "n must be"), (dict(n=1 << 31), "2^31"),
                     (dict(s=17), "cell_log2"), (dict(s=-9), "cell_log2"), (dict(X=None), "null"),
                     (dict(out=None), "null")):
        assert call(**kw) == -1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert call(n=0) == 0
    assert call(n=0, X=None, out=None) == 0
    assert call(n=0, G=1, H=1 << 15, W=(1 << 16) - 1, s=16) == 0          # G*H*W just below 2^31
    assert call(n=0, G=1, H=1 << 15, W=1 << 16) == -1
    assert lib.pcm_abi_version() == 8


def test_public_names():
    import pcm_amd
    from pcm_amd import _lib
    for name in ("height_grid", "HeightGrid"):
        assert name in pcm_amd.__all__ and getattr(pcm_amd, name) is not None
    assert "pcm_height_grid" in _lib.EXPORTS
    assert any(u.endswith("pcm_grid.hip") for u in _lib.UNITS)
    assert _lib.GRID_WORDS == 4 and _lib.GRID_MAXG == 256
    import torch
    with pytest.raises(_lib.PcmError):
        pcm_amd.height_grid(torch.zeros(4, 3), (2, 2))      # host tensor


# ---------------------------------------------------------------- the reference encoder itself
def cloud(n=4000, H=20, W=30, G=3, k=7, seed=3):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.normal(0, 5, n), rng.random(n) * H, rng.random(n) * W], axis=1).astype(np.float32)
    return X, rng.integers(0, k, n).astype(np.int32), rng.integers(0, G, n).astype(np.uint8)


@pytest.mark.parametrize("s", [0, 2, -1])
def test_encoder_matches_row_by_row_python(s):
    X, labels, groups = cloud()
    H, W, G, k = 20, 30, 3, 7
    q = GR.fixed_q(X[:, 0])
    words, (outside, skipped) = GR.encode(X, (H, W), q, s=s, labels=labels, k=k, groups=groups, n_groups=G)
    cells = GR.direct(X, (H, W), q, s=s, labels=labels, groups=groups, n_groups=G)
    assert skipped == 0 and outside == X.shape[0] - sum(len(v) for v in cells.values())
    assert (outside > 0) == (s < 0)
    want = np.zeros_like(words)
    for (g, fy, fx), rows in cells.items():
        zq = [r[0] for r in rows]
        want[g, 0, fy, fx] = len(rows)
        want[g, 1, fy, fx] = np.int64(sum(zq)).view(np.uint64)
        hi, lo = max(zq), min(zq)
        want[g, 2, fy, fx] = ((hi + GR.BIAS) << 32) | (GR.LOW - min(l for z, l in rows if z == hi))
        want[g, 3, fy, fx] = ((GR.BIAS - lo) << 32) | (GR.LOW - min(l for z, l in rows if z == lo))
    assert np.array_equal(words, want)
    # any order of the rows gives the same words
    p = np.random.default_rng(0).permutation(X.shape[0])
    again, _ = GR.encode(X[p], (H, W), q, s=s, labels=labels[p], k=k, groups=groups[p], n_groups=G)
    assert np.array_equal(again, words)


def test_encoder_edge_rows():
    H, W, k, G = 6, 9, 4, 2
    top = np.nextafter(np.float32(H), np.float32(0))
    X = np.array([[1, -0.0, 2], [1, -0.5, 2], [1, H, 2], [1, top, W - 1], [1, 2, -1e-3],
                  [np.nan, 1, 1], [1, np.inf, 1], [1, 1, 1], [1, 1, 1]], np.float32)
    labels = np.array([0, 0, 0, 0, 0, 0, 0, k, 0], np.int32)
    groups = np.array([0, 0, 0, 0, 0, 0, 0, 0, G], np.uint8)
    words, (outside, skipped) = GR.encode(X, (H, W), 20, labels=labels, k=k, groups=groups, n_groups=G)
    assert (int(words[:, 0].sum()), outside, skipped) == (2, 3, 4)
    assert words[0, 0, 0, 2] == 1 and words[0, 0, H - 1, W - 1] == 1


# ---------------------------------------------------------------- accessors
def test_accessors_on_numpy_words():
    from pcm_amd.grid import HeightGrid
    X, labels, groups = cloud()
    H, W, G, k = 20, 30, 3, 7
    q = GR.fixed_q(X[:, 0])
    words, _ = GR.encode(X, (H, W), q, labels=labels, k=k, groups=groups, n_groups=G)
    words[1, :, 4, 5] = 0                                              # an empty (group, pixel)
    hg = HeightGrid(words, q)
    assert hg.n_groups == G and hg.shape == (H, W) and hg.numpy().dtype == np.int64
    zq = np.ldexp(X[:, 0], q).astype(np.int64)
    fy, fx = X[:, 1].astype(int), X[:, 2].astype(int)
    cnt, sm = hg.counts(), hg.sums()
    assert cnt.dtype == np.int64 and sm.dtype == np.int64 and cnt.shape == (G, H, W)
    top, bot, tl, bl, mean, rel = hg.top(), hg.bottom(), hg.top_labels(), hg.bottom_labels(), hg.means(), hg.relief()
    assert top.dtype == np.float64 and tl.dtype == np.int32 and bl.dtype == np.int32
    seen = 0
    for g, y, x in np.ndindex(G, H, W):
        m = (groups == g) & (fy == y) & (fx == x)
        if (g, y, x) == (1, 4, 5) or not m.any():
            assert cnt[g, y, x] == 0 and tl[g, y, x] == -1 and np.isnan(top[g, y, x])
            continue
        seen += 1
        assert cnt[g, y, x] == m.sum() and sm[g, y, x] == zq[m].sum()
        assert top[g, y, x] == np.ldexp(float(zq[m].max()), -q) and bot[g, y, x] == np.ldexp(float(zq[m].min()), -q)
        assert tl[g, y, x] == labels[m][zq[m] == zq[m].max()].min()
        assert bl[g, y, x] == labels[m][zq[m] == zq[m].min()].min()
        assert mean[g, y, x] == np.ldexp(float(zq[m].sum()), -q) / m.sum()
        assert rel[g, y, x] == top[g, y, x] - bot[g, y, x] >= 0
    assert seen > 1000
    assert cnt[1, 4, 5] == 0 and sm[1, 4, 5] == 0 and tl[1, 4, 5] == -1 and bl[1, 4, 5] == -1
    assert np.isnan([top[1, 4, 5], bot[1, 4, 5], mean[1, 4, 5], rel[1, 4, 5]]).all()
    assert np.isfinite(mean[cnt > 0]).all() and (tl[cnt > 0] >= 0).all()
    assert (X[:, 0] < 0).any() and (sm < 0).any()                       # negative sums decode as int64
    with pytest.raises(ValueError):
        HeightGrid(words[:, :3], q)


def test_add_and_merged():
    from pcm_amd.grid import HeightGrid
    X, labels, groups = cloud()
    H, W, G, k = 20, 30, 3, 7
    q = GR.fixed_q(X[:, 0])
    kw = dict(origin=(0.5, -1.25), s=1)
    words, (outside, _) = GR.encode(X, (H, W), q, labels=labels, k=k, groups=groups, n_groups=G, **kw)
    h = 1500
    wa, (oa, _) = GR.encode(X[:h], (H, W), q, labels=labels[:h], k=k, groups=groups[:h], n_groups=G, **kw)
    wb, (ob, _) = GR.encode(X[h:], (H, W), q, labels=labels[h:], k=k, groups=groups[h:], n_groups=G, **kw)
    a, b = HeightGrid(wa, q, 1, (0.5, -1.25), oa), HeightGrid(wb, q, 1, (0.5, -1.25), ob)
    both = a + b
    assert np.array_equal(both.numpy().view(np.uint64), words) and both.outside == outside > 0
    u = lambda g: g.numpy().view(np.uint64)                             # noqa: E731
    assert np.array_equal(u(both)[:, :2], u(a)[:, :2] + u(b)[:, :2])
    assert np.array_equal(u(both)[:, 2:], np.maximum(u(a)[:, 2:], u(b)[:, 2:]))
    one, _ = GR.encode(X, (H, W), q, labels=labels, k=k, **kw)          # without groups
    mg = both.merged()
    assert mg.n_groups == 1 and np.array_equal(u(mg), one)
    assert np.array_equal(u(mg)[0, :2], u(both)[:, :2].sum(0, dtype=np.uint64))
    assert np.array_equal(u(mg)[0, 2:], u(both)[:, 2:].max(0))
    for other in (HeightGrid(wb, q + 1, 1, (0.5, -1.25)), HeightGrid(wb, q, 0, (0.5, -1.25)),
                  HeightGrid(wb, q, 1, (0.0, 0.0)), mg):
        with pytest.raises(ValueError):
            a + other


# ---------------------------------------------------------------- plugin
def oracle_fit_plugin(X, C0, max_iter, tol_abs):
    r = R.lloyd_fit(X, C0, max_iter=max_iter, tol=tol_abs)
    return r["labels"], r["centers"], r["inertia"], r["n_iter"]


def oracle_grid(X, labels, groups, k, G, shape, s, q):
    words, (outside, skipped) = GR.encode(np.ascontiguousarray(X, np.float32), shape, q, s=s, labels=labels, k=k,
                                          groups=groups, n_groups=G)
    assert skipped == 0
    return words.view(np.int64), outside


def three_days():
    """Three clouds over a 40 x 60 relief; the third covers only the left half and sits 0.5 higher."""
    rng = np.random.default_rng(4)
    out = []
    for day in range(3):
        yy, xx = np.mgrid[0:40, 0:60]
        keep = rng.random(yy.shape) > 0.2
        if day == 2:
            keep &= xx < 30
        z = 6 * np.sin(xx / 19.0) + 4 * np.cos(yy / 13.0) + rng.normal(0, 0.2, yy.shape) + (0.5 if day == 2 else 0.0)
        out.append(np.stack([z[keep], yy[keep].astype(np.float64), xx[keep].astype(np.float64)], axis=1))
    return out


def brute_layers(clouds, labels, centers, s):
    """The five arrays from the (dequantised) points, pixel by pixel."""
    X = np.concatenate(clouds).astype(np.float32)
    q = GR.fixed_q(X[:, 0])
    zq = np.ldexp(X[:, 0], q).astype(np.int64)
    g = np.repeat(np.arange(len(clouds)), [c.shape[0] for c in clouds])
    fy = np.floor(X[:, 1] / 2.0 ** s).astype(int)
    fx = np.floor(X[:, 2] / 2.0 ** s).astype(int)
    H, W = fy.max() + 1, fx.max() + 1
    hmap, spread, surf = np.full((H, W), np.nan), np.zeros((H, W)), np.full((H, W), np.nan)
    cover, elem = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    for y in range(H):
        for x in range(W):
            m = (fy == y) & (fx == x)
            if not m.any():
                continue
            hmap[y, x] = np.ldexp(float(zq[m].sum()), -q) / m.sum()
            days = [np.ldexp(float(zq[m & (g == d)].sum()), -q) / (m & (g == d)).sum() for d in np.unique(g[m])]
            cover[y, x] = len(days)
            spread[y, x] = max(days) - min(days) if len(days) >= 2 else 0.0
            j = labels[m][zq[m] == zq[m].max()].min()
            surf[y, x], elem[y, x] = float(centers[j, 0]), j + 1
    return [hmap, spread, cover, surf, elem]


@pytest.mark.parametrize("s", [0, 2])
def test_kmeans_fuse_height_map(s):
    import pcm_amd
    clouds = three_days()
    k = 12
    base_layers, base = pcm_amd.kmeans_fuse(clouds + [np.zeros((0, 3))], n_clusters=k, fit=oracle_fit_plugin)
    layers, res = pcm_amd.kmeans_fuse(clouds + [np.zeros((0, 3))], n_clusters=k, fit=oracle_fit_plugin, height_map=True,
                                      height_map_cell_log2=s, grid=oracle_grid)
    # default output unchanged: the first two layers and the rest of the result
    assert len(base_layers) == 2 and set(base) == {"labels", "centers", "inertia", "n_iter", "n_points"}
    assert set(res) == set(base) | {"height_map"}
    for key in base:
        np.testing.assert_array_equal(res[key], base[key])
    for a, b in zip(layers[:2], base_layers):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[2] == b[2] and a[1]["name"] == b[1]["name"] and set(a[1]["properties"]) == set(b[1]["properties"])
    assert [l[1]["name"] for l in layers[2:]] == [PREFIX + n for n in NAMES]
    assert [l[2] for l in layers[2:]] == ["image"] * 4 + ["labels"]
    assert all(l[1]["scale"] == (2.0 ** s, 2.0 ** s) for l in layers[2:])
    H, W = 39 // 2 ** s + 1, 59 // 2 ** s + 1
    hm = res["height_map"]
    assert set(hm) == {"words", "q", "cell_log2", "origin", "shape", "outside", "sizes"}
    X = np.concatenate(clouds).astype(np.float32)
    assert hm["shape"] == (H, W) and hm["cell_log2"] == s and hm["origin"] == (0.0, 0.0) and hm["outside"] == 0
    assert hm["sizes"] == [c.shape[0] for c in clouds] and hm["q"] == GR.fixed_q(X[:, 0])
    assert hm["words"].shape == (3, 4, H, W) and hm["words"].dtype == np.int64
    want = brute_layers(clouds, res["labels"], res["centers"], s)
    for (data, params, kind), w in zip(layers[2:], want):
        assert data.shape == (H, W)
        np.testing.assert_array_equal(data, w, err_msg=params["name"])
    assert layers[6][0].dtype == np.int32 and layers[4][0].max() == 3 and layers[4][0].min() <= 2
    if s == 0:
        assert np.isnan(layers[2][0]).any() and (layers[6][0] == 0).any()      # empty pixels: NaN / background
        assert layers[4][0][:, 30:].max() == 2                                # the third day misses the right half
    # where the raised third day is seen the clouds disagree by more than the noise
    assert np.median(layers[3][0][layers[4][0] == 3]) > 0.2
    # one cloud: nothing to spread
    l1, _ = pcm_amd.kmeans_fuse(clouds[:1], n_clusters=k, fit=oracle_fit_plugin, height_map=True, grid=oracle_grid)
    assert not l1[3][0].any() and l1[4][0].max() == 1


def test_kmeans_fuse_height_map_limits():
    import pcm_amd
    clouds = three_days()
    with pytest.raises(ValueError, match="height_map_cell_log2"):       # 3 x 10240 x 15360 x 32 B = 14 GiB
        pcm_amd.kmeans_fuse(clouds, n_clusters=4, fit=oracle_fit_plugin, height_map=True, height_map_cell_log2=-8,
                            grid=oracle_grid)
    with pytest.raises(ValueError, match="height_map_cell_log2"):
        pcm_amd.kmeans_fuse(clouds, n_clusters=4, fit=oracle_fit_plugin, height_map=True, height_map_cell_log2=17,
                            grid=oracle_grid)
    rng = np.random.default_rng(0)
    many = [rng.random((2, 3)) for _ in range(257)]
    with pytest.raises(ValueError, match="256"):
        pcm_amd.kmeans_fuse(many, n_clusters=4, fit=oracle_fit_plugin, height_map=True, grid=oracle_grid)
    layers, res = pcm_amd.kmeans_fuse(many[:256], n_clusters=4, fit=oracle_fit_plugin, height_map=True, grid=oracle_grid)
    assert res["height_map"]["words"].shape == (256, 4, 1, 1) and layers[4][0][0, 0] == 256
    # points at negative y or x lie outside the raster, whose origin is (0, 0)
    shifted = [clouds[0] - np.array([0.0, 5.0, 0.0])]
    _, r2 = pcm_amd.kmeans_fuse(shifted, n_clusters=4, fit=oracle_fit_plugin, height_map=True, grid=oracle_grid)
    assert r2["height_map"]["shape"] == (35, 60) and r2["height_map"]["outside"] == int((shifted[0][:, 1] < 0).sum()) > 0


def test_extractor_passes_height_map():
    from fake_pipeline import SyntheticPairExtractor, SyntheticStages
    from oracle import cloud_ref
    import pcm_amd

    def oracle_assemble(disparity, validity):
        return cloud_ref.assemble(disparity, validity)[:2]

    base = SyntheticPairExtractor(n_pairs=2, shape=(40, 50))
    out0 = pcm_amd.HeightMapExtractor(base=base, n_clusters=8, fit=oracle_fit_plugin).run("roi.kml")
    ext = pcm_amd.HeightMapExtractor(base=base, n_clusters=8, fit=oracle_fit_plugin, height_map=True,
                                     height_map_cell_log2=1, grid=oracle_grid)
    out = ext.run("roi.kml")
    assert len(out) == len(out0) + 5 and "height_map" in ext.last_result
    assert [l[1]["name"] for l in out[-5:]] == [PREFIX + n for n in NAMES]
    assert out[-1][0].shape == (20, 25) and out[-1][1]["scale"] == (2.0, 2.0)
    # the stages route
    kw = dict(n_clusters=8, fit=oracle_fit_plugin, _assemble=oracle_assemble)
    st0 = pcm_amd.HeightMapExtractor(stages=SyntheticStages(n_pairs=2, shape=(40, 50)), **kw).run("roi.kml")
    ext2 = pcm_amd.HeightMapExtractor(stages=SyntheticStages(n_pairs=2, shape=(40, 50)), height_map=True, grid=oracle_grid,
                                      **kw)
    st = ext2.run("roi.kml")
    assert len(st) == len(st0) + 5 and [l[1]["name"] for l in st[-5:]] == [PREFIX + n for n in NAMES]
    assert st[-3][0].max() == 2 and ext2.last_result["height_map"]["cell_log2"] == 0
    # the size limit comes back as the reference's error layer, never as an exception
    for route in (dict(base=base), dict(stages=SyntheticStages(n_pairs=2, shape=(40, 50)), _assemble=oracle_assemble)):
        err = pcm_amd.HeightMapExtractor(n_clusters=8, fit=oracle_fit_plugin, height_map=True, height_map_cell_log2=-8,
                                         grid=oracle_grid, **route).run("roi.kml")
        assert len(err) == 1 and err[0][2] == "image" and err[0][1]["name"].startswith("Error:")
        assert "height_map_cell_log2" in err[0][1]["name"]
