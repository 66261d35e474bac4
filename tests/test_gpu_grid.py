"""GPU: ``pcm_height_grid`` and everything built on it, bitwise on all four planes
and both trailing words against the NumPy reference encoder (tests/grid_ref.py):
whether a row's words were combined over a run of lanes by the segmented scan or
went out as its own atomics, the integer words must be the same bit pattern.
"""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import grid_ref as GR  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pcm_amd
    from pcm_amd import _lib
    _lib.load()
    return pcm_amd


def raw(X, shape, q, *, origin=(0.0, 0.0), s=0, labels=None, k=1, groups=None, G=1, buf=None, blocks=None):
    """pcm_height_grid itself: uint64 words (G, 4, H, W), (outside, skipped), and the device buffer."""
    from pcm_amd import _lib
    lib = _lib.load()
    n = X.shape[0]
    H, W = shape
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
    lt = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    gt = None if groups is None else torch.from_numpy(np.ascontiguousarray(groups, dtype=np.uint8)).cuda()
    if buf is None:
        buf = torch.zeros(G * 4 * H * W + 2, dtype=torch.int64, device="cuda")
    if blocks is not None:
        os.environ["PCM_GRID_BLOCKS"] = str(blocks)
    try:
        rc = lib.pcm_height_grid(ctypes.c_void_p(Xt.data_ptr()), n, None if lt is None else ctypes.c_void_p(lt.data_ptr()), k,
                                 None if gt is None else ctypes.c_void_p(gt.data_ptr()), G, H, W, origin[0], origin[1], s,
                                 q, ctypes.c_void_p(buf.data_ptr()),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    finally:
        os.environ.pop("PCM_GRID_BLOCKS", None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint64)
    return host[:-2].reshape(G, 4, H, W).copy(), (int(host[-2]), int(host[-1])), buf


def same(got, want, where=""):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and bad.size == 0, \
        f"{where}: {bad.shape[0]} words differ, first (g, w, y, x) {bad[:6].tolist()}: " \
        f"got {[hex(int(got[tuple(b)])) for b in bad[:3]]} want {[hex(int(want[tuple(b)])) for b in bad[:3]]}"


H1, W1, G1, K1 = 37, 150, 3, 7


@pytest.fixture(scope="module")
def raster():
    """Three clouds over a 37 x 150 image with ~70 % valid pixels, each a random 80 % of them in
    raster order, concatenated; labels in [0, 7); z of both signs.  With the reference words per s."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H1, 0:W1]
    valid = rng.random((H1, W1)) < 0.7
    X, groups = [], []
    for day in range(G1):
        keep = valid & (rng.random((H1, W1)) < 0.8)
        z = 6 * np.sin(xx / 19.0) + 4 * np.cos(yy / 13.0) + rng.normal(0, 0.3, yy.shape) + 0.5 * day - 1.0
        X.append(np.stack([z[keep], yy[keep], xx[keep]], axis=1))
        groups.append(np.full(int(keep.sum()), day, np.uint8))
    X = np.concatenate(X).astype(np.float32)
    groups = np.concatenate(groups)
    labels = rng.integers(0, K1, X.shape[0]).astype(np.int32)
    assert (X[:, 0] > 0).any() and (X[:, 0] < 0).any() and X.shape[0] % 64 != 0
    q = GR.fixed_q(X[:, 0])
    want = {s: GR.encode(X, (H1, W1), q, s=s, labels=labels, k=K1, groups=groups, n_groups=G1) for s in (0, 2, -1)}
    return X, labels, groups, q, want


# ---------------------------------------------------------------- 1. raster cloud
@pytest.mark.parametrize("s", [0, 2, -1])
def test_raster_cloud(pcm, raster, s):
    X, labels, groups, q, want = raster
    words, (outside, skipped) = want[s]
    assert skipped == 0 and (outside > X.shape[0] // 2) == (s == -1)
    got, trail, _ = raw(X, (H1, W1), q, s=s, labels=labels, k=K1, groups=groups, G=G1)
    assert trail == (outside, 0)
    same(got, words, f"s={s}")
    # the public wrapper: default q, groups of any integer dtype
    hg = pcm.height_grid(torch.from_numpy(X).cuda(), (H1, W1), cell_log2=s, labels=torch.from_numpy(labels).cuda(),
                         n_clusters=K1, groups=torch.from_numpy(groups.astype(np.int64)).cuda(), n_groups=G1)
    assert hg.q == q and hg.cell_log2 == s and hg.outside == outside and hg.origin == (0.0, 0.0)
    assert hg.words.is_cuda and hg.words.dtype == torch.int64 and tuple(hg.words.shape) == (G1, 4, H1, W1)
    same(hg.numpy().view(np.uint64), words, f"wrapper s={s}")


# ---------------------------------------------------------------- 2. order and grid independence
@pytest.mark.parametrize("s", [0, 2])
def test_order_and_grid_independence(pcm, raster, s):
    X, labels, groups, q, want = raster
    p = np.random.default_rng(2).permutation(X.shape[0])
    for blocks in (None, 3):
        got, trail, _ = raw(X[p], (H1, W1), q, s=s, labels=labels[p], k=K1, groups=groups[p], G=G1, blocks=blocks)
        assert trail == want[s][1]
        same(got, want[s][0], f"permuted, blocks={blocks}")
    got, _, _ = raw(X, (H1, W1), q, s=s, labels=labels, k=K1, groups=groups, G=G1, blocks=3)
    same(got, want[s][0], "raster order, 3 blocks")


# ---------------------------------------------------------------- 3. runs over the wave edges
def test_runs_over_wave_edges(pcm):
    """Rows ordered as runs of equal cell whose lengths cycle through 1, 3, 63, 64, 65, 130 at s = 2:
    runs that end at, start at and straddle lane 63 -> 0 and whole rounds."""
    rng = np.random.default_rng(3)
    H, W, k, s = 16, 24, 5, 2
    lengths = [1, 3, 63, 64, 65, 130]
    cells, rows = [], []
    for t in range(60):
        L = lengths[t % len(lengths)]
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        while cells and cells[-1] == (cy, cx):                  # adjacent runs differ in their cell
            cy, cx = rng.integers(0, H), rng.integers(0, W)
        cells.append((cy, cx))
        yx = np.array([cy, cx]) * 4 + rng.random((L, 2)) * 3.9
        rows.append(np.concatenate([rng.normal(0, 3, (L, 1)), yx], axis=1))
    X = np.concatenate(rows).astype(np.float32)
    assert X.shape[0] == 10 * sum(lengths)
    labels = rng.integers(0, k, X.shape[0]).astype(np.int32)
    q = GR.fixed_q(X[:, 0])
    want, (outside, skipped) = GR.encode(X, (H, W), q, s=s, labels=labels, k=k)
    assert (outside, skipped) == (0, 0) and int(want[0, 0].max()) >= 130
    got, trail, _ = raw(X, (H, W), q, s=s, labels=labels, k=k)
    assert trail == (0, 0)
    same(got, want, "runs")
    got, _, _ = raw(X, (H, W), q, s=s, labels=labels, k=k, blocks=1)
    same(got, want, "runs, one block")


# ---------------------------------------------------------------- 4. one cell
def test_one_cell(pcm):
    n = 5000
    zmax = np.float32(8 - 2.0 ** -21)
    X = np.empty((n, 3), np.float32)
    X[:, 0] = np.where(np.arange(n) % 2 == 0, zmax, -zmax)
    X[:, 1:] = (3.5, 5.25)
    labels = (np.arange(n) % 2).astype(np.int32)               # label 0 on top, label 1 at the bottom
    q = GR.fixed_q(X[:, 0])
    assert q == 22 and int(np.ldexp(zmax, q)) == (1 << 25) - 2
    want, _ = GR.encode(X, (8, 8), q, labels=labels, k=2)
    got, trail, _ = raw(X, (8, 8), q, labels=labels, k=2)
    assert trail == (0, 0)
    same(got, want, "one cell")
    from pcm_amd.grid import HeightGrid
    hg = HeightGrid(got, q)
    assert hg.counts()[0, 3, 5] == n and hg.sums()[0, 3, 5] == 0 and int(hg.counts().sum()) == n
    assert hg.top()[0, 3, 5] == float(zmax) and hg.bottom()[0, 3, 5] == -float(zmax)
    assert hg.top_labels()[0, 3, 5] == 0 and hg.bottom_labels()[0, 3, 5] == 1
    assert not np.delete(got.reshape(4, 64), 3 * 8 + 5, axis=1).any()


# ---------------------------------------------------------------- 5. top tie
def test_top_tie_goes_to_the_smaller_label(pcm):
    from pcm_amd.grid import HeightGrid
    X = np.array([[1.5, 2.0, 3.0], [1.5, 2.5, 3.5]], np.float32)
    for labels in ([5, 2], [2, 5]):
        got, _, _ = raw(X, (4, 4), 20, labels=np.array(labels, np.int32), k=6)
        same(got, GR.encode(X, (4, 4), 20, labels=labels, k=6)[0], f"labels {labels}")
        hg = HeightGrid(got, 20)
        assert hg.counts()[0, 2, 3] == 2 and hg.top_labels()[0, 2, 3] == 2 and hg.bottom_labels()[0, 2, 3] == 2
        assert hg.top()[0, 2, 3] == 1.5 == hg.bottom()[0, 2, 3]


# ---------------------------------------------------------------- 6. edge rows
def test_edge_rows(pcm):
    H, W, k, G = 6, 9, 4, 2
    top = np.nextafter(np.float32(H), np.float32(0))
    X = np.array([[1, -0.0, 2], [1, -0.5, 2], [1, H, 2], [1, top, W - 1], [1, 2, -1e-3],
                  [np.nan, 1, 1], [1, np.inf, 1], [1, 1, 1], [1, 1, 1]], np.float32)
    labels = np.array([0, 0, 0, 0, 0, 0, 0, k, 0], np.int32)
    groups = np.array([0, 0, 0, 0, 0, 0, 0, 0, G], np.uint8)
    want, (outside, skipped) = GR.encode(X, (H, W), 20, labels=labels, k=k, groups=groups, n_groups=G)
    assert (int(want[:, 0].sum()), outside, skipped) == (2, 3, 4)
    got, trail, _ = raw(X, (H, W), 20, labels=labels, k=k, groups=groups, G=G)
    assert trail == (3, 4)
    same(got, want, "edge rows")
    assert got[0, 0, 0, 2] == 1 and got[0, 0, H - 1, W - 1] == 1
    # |zq| >= 2^25 is skipped too: z = 32 at q = 20
    X2 = np.array([[32.0, 1, 1], [-32.0, 1, 1], [np.nextafter(np.float32(32), np.float32(0)), 1, 1]], np.float32)
    got2, trail2, _ = raw(X2, (H, W), 20)
    assert trail2 == (0, 2) and got2[0, 0, 1, 1] == 1
    same(got2, GR.encode(X2, (H, W), 20)[0], "height bound")
    # the wrapper raises on skipped rows and checks the groups itself
    Xt, lt = torch.from_numpy(X).cuda(), torch.from_numpy(labels).cuda()
    with pytest.raises(ValueError, match="skipped 3 rows"):
        pcm.height_grid(Xt[:8], (H, W), labels=lt[:8], n_clusters=k, q=20)
    with pytest.raises(ValueError, match="groups must lie"):
        pcm.height_grid(Xt, (H, W), labels=lt, n_clusters=k, groups=torch.from_numpy(groups).cuda(), n_groups=G, q=20)
    ok = pcm.height_grid(Xt[:5], (H, W), labels=lt[:5], n_clusters=k, q=20)
    assert ok.outside == 3 and int(ok.counts().sum()) == 2


# ---------------------------------------------------------------- 7. origin and accumulation
def test_origin_and_accumulation(pcm, raster):
    X, labels, groups, q, _ = raster
    X = X + np.float32([0, 10.25, -3.5])
    kw = dict(origin=(10.25, -3.5), cell_log2=1)
    H, W = 19, 75
    want, (outside, _) = GR.encode(X, (H, W), q, origin=(10.25, -3.5), s=1, labels=labels, k=K1, groups=groups, n_groups=G1)
    assert outside == 0 and want[:, 0, H - 1].any() and want[:, 0, :, W - 1].any()
    Xt, lt, gt = torch.from_numpy(X).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(groups).cuda()
    whole = pcm.height_grid(Xt, (H, W), labels=lt, n_clusters=K1, groups=gt, n_groups=G1, **kw)
    same(whole.numpy().view(np.uint64), want, "one call")
    h = 4321
    part = pcm.height_grid(Xt[:h], (H, W), labels=lt[:h], n_clusters=K1, groups=gt[:h], n_groups=G1, q=q, **kw)
    back = pcm.height_grid(Xt[h:], (H, W), labels=lt[h:], n_clusters=K1, groups=gt[h:], n_groups=G1, out=part, **kw)
    assert back is part
    same(part.numpy().view(np.uint64), want, "two chunks through out=")
    # one call per day, then + ; merged() against the grid built without groups
    one = GR.encode(X, (H, W), q, origin=(10.25, -3.5), s=1, labels=labels, k=K1)[0]
    days = [pcm.height_grid(Xt[gt == g], (H, W), labels=lt[gt == g], n_clusters=K1, q=q, **kw) for g in range(G1)]
    same((days[0] + days[1] + days[2]).numpy().view(np.uint64), one, "a + b of the days")
    same((days[0] + days[1]).numpy().view(np.uint64),
         GR.encode(X[groups < 2], (H, W), q, origin=(10.25, -3.5), s=1, labels=labels[groups < 2], k=K1)[0], "two days")
    for g in range(G1):
        same(days[g].numpy().view(np.uint64), want[g:g + 1], f"day {g}")
    same(whole.merged().numpy().view(np.uint64), one, "merged")
    same(pcm.height_grid(Xt, (H, W), labels=lt, n_clusters=K1, q=q, **kw).numpy().view(np.uint64), one, "no groups")
    with pytest.raises(ValueError):
        pcm.height_grid(Xt, (H, W), labels=lt, n_clusters=K1, groups=gt, n_groups=G1, q=q + 1, out=part, **kw)
    with pytest.raises(ValueError):
        pcm.height_grid(Xt, (H, W), labels=lt, n_clusters=K1, groups=gt, n_groups=G1, origin=(0, 0), cell_log2=1, out=part)


# ---------------------------------------------------------------- 8. empty cloud
def test_empty_cloud(pcm):
    hg = pcm.height_grid(torch.zeros((0, 3), device="cuda"), (5, 7), n_groups=2)
    assert tuple(hg.words.shape) == (2, 4, 5, 7) and not hg.words.any() and hg.outside == 0
    assert np.isnan(hg.means()).all() and (hg.top_labels() == -1).all()


# ---------------------------------------------------------------- 9. plugin on the device path
def test_plugin_height_map_end_to_end(pcm):
    from pcm_amd.grid import HeightGrid
    rng = np.random.default_rng(31)
    clouds = []
    for day in range(3):
        yy, xx = np.mgrid[0:40, 0:60]
        keep = rng.random(yy.shape) > 0.2
        if day == 2:
            keep &= xx < 30
        z = 6 * np.sin(xx / 19.0) + 4 * np.cos(yy / 13.0) + rng.normal(0, 0.2, yy.shape) + 0.5 * day
        clouds.append(np.stack([z[keep], yy[keep].astype(np.float64), xx[keep].astype(np.float64)], axis=1))
    k = 16
    base_layers, base = pcm.kmeans_fuse(clouds, k)
    layers, res = pcm.kmeans_fuse(clouds, k, height_map=True)
    assert len(base_layers) == 2 and len(layers) == 7 and set(res) == set(base) | {"height_map"}
    for key in base:
        np.testing.assert_array_equal(res[key], base[key])
    for a, b in zip(layers[:2], base_layers):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[2] == b[2] and a[1]["name"] == b[1]["name"]
        for pk in b[1]["properties"]:
            np.testing.assert_array_equal(a[1]["properties"][pk], b[1]["properties"][pk])
    X = np.concatenate(clouds).astype(np.float32)
    sizes = [c.shape[0] for c in clouds]
    q = GR.fixed_q(X[:, 0])
    want, (outside, skipped) = GR.encode(X, (40, 60), q, labels=res["labels"], k=k, groups=np.repeat(np.arange(3), sizes),
                                         n_groups=3)
    hm = res["height_map"]
    assert (outside, skipped) == (0, 0) and hm["outside"] == 0 and hm["shape"] == (40, 60) and hm["q"] == q
    assert hm["sizes"] == sizes and hm["cell_log2"] == 0 and hm["origin"] == (0.0, 0.0)
    same(hm["words"].view(np.uint64), want, "kmeans_fuse height_map")
    # the five arrays from the reference words, the centres and nothing else
    cnt = want[:, 0].astype(np.int64)
    sm = want[:, 1].view(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        hmap = np.where(cnt.sum(0) > 0, np.ldexp(sm.sum(0).astype(np.float64), -q) / cnt.sum(0), np.nan)
        per = np.where(cnt > 0, np.ldexp(sm.astype(np.float64), -q) / cnt, np.nan)
        spread = np.where((cnt > 0).sum(0) >= 2, np.nanmax(np.nan_to_num(per, nan=-np.inf), axis=0) -
                          np.nanmin(np.nan_to_num(per, nan=np.inf), axis=0), 0.0)
    topw = want[:, 2].max(0)
    lab = np.where(topw != 0, 0xFFFFFFFF - (topw & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    surf = np.where(lab >= 0, res["centers"].astype(np.float64)[np.maximum(lab, 0), 0], np.nan)
    names = ["Fused Height Map", "Fused Height Spread", "Fused Coverage", "Fused Surface Height", "Fused Surface Elements"]
    assert [l[1]["name"] for l in layers[2:]] == ["[Multi-day 3D Point Cloud] " + nm for nm in names]
    assert [l[2] for l in layers[2:]] == ["image"] * 4 + ["labels"] and all(l[1]["scale"] == (1.0, 1.0) for l in layers[2:])
    for (data, params, _), w in zip(layers[2:], [hmap, spread, (cnt > 0).sum(0), surf, lab + 1]):
        np.testing.assert_array_equal(data, w, err_msg=params["name"])
    assert layers[6][0].dtype == np.int32 and np.isnan(layers[2][0]).any() and layers[4][0][:, 30:].max() == 2
    assert np.array_equal(HeightGrid(want, q).merged().top_labels()[0], lab)
    # clouds already on the device give the same words
    dev = [torch.from_numpy(c).cuda() for c in clouds]
    _, res_d = pcm.kmeans_fuse(clouds, k, height_map=True, device_clouds=dev)
    same(res_d["height_map"]["words"].view(np.uint64), want, "device clouds")
