"""GPU: ``pcm_cluster_stats`` and everything built on it, bitwise on all W words
of every (group, cluster) row against the NumPy reference encoder
(tests/stats_ref.py): whichever accumulation path a row takes -- the wave
reduction carried over a run of equal keys, or the per-lane atomics of
stragglers -- the integer words must be the same bit pattern.
"""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import stats_ref as SR  # noqa: E402
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


def raw(X, labels, k, q, groups=None, G=1, dtype=torch.float32, buf=None):
    """pcm_cluster_stats itself: uint64 words (G, K, W), the skipped word, and the device buffer."""
    from pcm_amd import _lib
    lib = _lib.load()
    n, d = X.shape
    W = SR.words_per_row(d)
    Xt = torch.from_numpy(np.ascontiguousarray(X)).to("cuda", dtype)
    lt = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    gt = None if groups is None else torch.from_numpy(np.ascontiguousarray(groups, dtype=np.uint8)).cuda()
    if buf is None:
        buf = torch.zeros(G * k * W + 1, dtype=torch.int64, device="cuda")
    qa = np.ascontiguousarray(q, dtype=np.int32)
    rc = lib.pcm_cluster_stats(ctypes.c_void_p(Xt.data_ptr()), 1 if dtype == torch.float16 else 0, n, d,
                               ctypes.c_void_p(lt.data_ptr()), None if gt is None else ctypes.c_void_p(gt.data_ptr()),
                               G, k, qa.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(buf.data_ptr()),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint64)
    return host[:-1].reshape(G, k, W).copy(), int(host[-1]), buf


def same(got, want, where=""):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and bad.size == 0, \
        f"{where}: {bad.shape[0]} words differ, first (g, j, w) {bad[:6].tolist()}: " \
        f"got {[hex(int(got[tuple(b)])) for b in bad[:3]]} want {[hex(int(want[tuple(b)])) for b in bad[:3]]}"


def blobs(n, d, seed, nb=12, sd=0.8, shift=-3.0):
    rng = np.random.default_rng(seed)
    centers = rng.random((nb, d)) * 10 + shift
    return (centers[rng.integers(0, nb, n)] + rng.normal(0, sd, (n, d))).astype(np.float32)


def run_order(key, lengths=(37, 64, 100)):
    """A row order made of runs of equal key whose lengths cycle through
    ``lengths`` (runs that straddle the 64-row wave rounds)."""
    order = np.argsort(key, kind="stable")
    sk = key[order]
    starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    ends = np.r_[starts[1:], sk.size]
    pos = starts.copy()
    out, t, live = [], 0, list(range(starts.size))
    while live:
        nxt = []
        for s in live:
            L = lengths[t % len(lengths)]
            t += 1
            e = min(pos[s] + L, ends[s])
            out.append(order[pos[s]:e])
            pos[s] = e
            if e < ends[s]:
                nxt.append(s)
        live = nxt
    return np.concatenate(out)


# ---------------------------------------------------------------- 1. blobs, three row orders
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("k", [1, 16, 300])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_blobs_three_orders(pcm, d, k, G):
    n = 50_000
    X = blobs(n, d, 100 * d + k + G)
    labels = R.assign(X, X[R.init_indices(n, k)])
    groups = np.random.default_rng(7).integers(0, G, n)
    q = R.fixed_q(X)
    want, skipped = SR.encode(X, labels, k, q, groups, G)
    assert skipped == 0
    key = groups * k + labels
    orders = {"random": np.arange(n), "sorted": np.argsort(key, kind="stable"), "runs": run_order(key)}
    assert sorted(orders["runs"].tolist()) == list(range(n))
    for name, o in orders.items():
        got, sk, _ = raw(X[o], labels[o], k, q, groups[o] if G > 1 else None, G)
        assert sk == 0
        same(got, want, f"d={d} k={k} G={G} {name}")
    # the public wrapper: default q = the fit's exponents, groups of any integer dtype
    st = pcm.cluster_stats(torch.from_numpy(X).cuda(), torch.from_numpy(labels).cuda(), k,
                           groups=torch.from_numpy(groups).cuda(), n_groups=G)
    assert st.q == list(q) and st.d == d and tuple(st.words.shape) == (G, k, SR.words_per_row(d))
    assert st.words.is_cuda and st.words.dtype == torch.int64
    same(st.numpy().view(np.uint64), want, "wrapper")


# ---------------------------------------------------------------- 2. sizes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 50_001])
def test_sizes(pcm, n):
    k, G = 16, 3
    X = blobs(max(n, k), 3, n)[:n]
    labels = R.assign(X, blobs(k, 3, 1))
    groups = np.random.default_rng(n).integers(0, G, n)
    q = R.fixed_q(X)
    want, _ = SR.encode(X, labels, k, q, groups, G)
    for name, o in (("random", np.arange(n)), ("sorted", np.argsort(groups * k + labels, kind="stable"))):
        got, sk, _ = raw(X[o], labels[o], k, q, groups[o], G)
        assert sk == 0
        same(got, want, f"n={n} {name}")


def test_empty_cloud(pcm):
    st = pcm.cluster_stats(torch.zeros((0, 3), device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), 4)
    assert tuple(st.words.shape) == (1, 4, 16) and not st.words.any()


# ---------------------------------------------------------------- 3. signs and magnitudes
@pytest.mark.parametrize("case", ["mixed", "negative", "ulp_below_pow2"])
def test_signs_and_magnitudes(pcm, case):
    n, k, G = 20_000, 16, 2
    rng = np.random.default_rng(5)
    if case == "mixed":
        X = blobs(n, 3, 3, shift=-5.0)
        assert (X > 0).any() and (X < 0).any()
    elif case == "negative":
        X = blobs(n, 3, 4, shift=-40.0)
        assert (X < 0).all()
    else:
        # max|x_a| one ulp below 2^4: |xq| = 2^25 - 2, products just below 2^50, of both signs
        top = np.nextafter(np.float32(16.0), np.float32(0.0))
        X = (rng.random((n, 3)) * 32 - 16).astype(np.float32)
        X[::7] = np.where(rng.random((X[::7].shape[0], 3)) < 0.5, top, -top)
        X = np.clip(X, -top, top)
    labels = rng.integers(0, k, n).astype(np.int32)
    labels[: n // 2] = np.sort(labels[: n // 2])          # half in long runs, half stragglers
    groups = rng.integers(0, G, n)
    q = R.fixed_q(X)
    if case == "ulp_below_pow2":
        assert list(q) == [21, 21, 21] and int(np.abs(R.to_fixed(X, q)).max()) == (1 << 25) - 2
    want, _ = SR.encode(X, labels, k, q, groups, G)
    if case != "negative":
        assert (want.view(np.int64)[..., 5::2] < 0).any()          # negative hi-limb sums
    got, sk, _ = raw(X, labels, k, q, groups, G)
    assert sk == 0
    same(got, want, case)


def test_one_row_takes_300000_points(pcm):
    """Every wave adds into one (g, j): negative hi-limb sums, lo sums far above 2^32."""
    n, k, G = 300_000, 8, 3
    rng = np.random.default_rng(6)
    X = (rng.random((n, 3)) * np.float32([60, 60, 60]) - np.float32([0, 60, 30])).astype(np.float32)   # +, -, mixed
    labels = np.full(n, 5, np.int32)
    groups = np.full(n, 2, np.uint8)
    q = R.fixed_q(X)
    want, _ = SR.encode(X, labels, k, q, groups, G)
    row = want[2, 5]
    assert int(row[0]) == n and int(row[4]) > 1 << 40                     # lo of xx: about n * 2^31
    assert int(row.view(np.int64)[7]) < 0                                 # hi of x*y: x > 0 > y
    got, sk, _ = raw(X, labels, k, q, groups, G)
    assert sk == 0
    same(got, want, "one row")
    assert not np.delete(got.reshape(-1, 16), 2 * k + 5, axis=0).any()


# ---------------------------------------------------------------- 4. fp16
def test_fp16_d4_golden(pcm):
    g = np.load(os.path.join(GOLDEN, "d4_fp16.npz"))
    X, labels = g["X"], g["fit_labels"]
    assert np.array_equal(X.astype(np.float16).astype(np.float32), X)      # widened exactly
    k = g["fit_centers"].shape[0]
    q = R.fixed_q(X)
    groups = (np.arange(X.shape[0]) // 1500).astype(np.uint8)
    want, _ = SR.encode(X, labels, k, q, groups, 3)
    got, sk, _ = raw(X, labels, k, q, groups, 3, dtype=torch.float16)
    assert sk == 0
    same(got, want, "d4_fp16")
    st = pcm.cluster_stats(torch.from_numpy(X).to("cuda", torch.float16), torch.from_numpy(labels).cuda(), k)
    same(st.numpy().view(np.uint64), SR.encode(X, labels, k, q)[0], "d4_fp16 wrapper")
    want_c = R.average(st.sums()[0], st.counts()[0], q, g["fit_centers"])
    assert np.array_equal(st.means()[0].astype(np.float32)[st.counts()[0] > 0], want_c[st.counts()[0] > 0])


# ---------------------------------------------------------------- 5. skipped rows
def test_skipped_rows(pcm):
    n, k, G = 10_000, 16, 3
    rng = np.random.default_rng(8)
    X = blobs(n, 3, 8)
    labels = np.sort(rng.integers(0, k, n)).astype(np.int32)
    groups = rng.integers(0, G, n).astype(np.uint8)
    q = R.fixed_q(X)
    bad = rng.choice(n, 500, replace=False)
    labels[bad[:100]] = -1
    labels[bad[100:200]] = k
    groups[bad[200:300]] = G
    X[bad[300:400], rng.integers(0, 3, 100)] = np.nan
    X[bad[400:450], rng.integers(0, 3, 50)] = np.inf
    X[bad[450:], rng.integers(0, 3, 50)] = -np.inf
    labels[bad[300]] = -5                                               # two reasons: still one skipped row
    want, want_skipped = SR.encode(X, labels, k, q, groups, G)
    assert want_skipped == 500
    got, sk, _ = raw(X, labels, k, q, groups, G)
    assert sk == 500
    same(got, want, "skipping")
    assert int(got[..., 0].sum()) == n - 500
    # the wrapper raises and gives the count
    Xt, lt = torch.from_numpy(X).cuda(), torch.from_numpy(labels).cuda()
    ok = groups < G
    with pytest.raises(ValueError, match="skipped 400 rows"):
        pcm.cluster_stats(Xt[torch.from_numpy(ok).cuda()], lt[torch.from_numpy(ok).cuda()], k, q=list(q),
                          groups=torch.from_numpy(groups[ok]).cuda(), n_groups=G)
    with pytest.raises(ValueError, match="groups must lie"):
        pcm.cluster_stats(Xt, lt, k, q=list(q), groups=torch.from_numpy(groups).cuda(), n_groups=G)
    with pytest.raises(ValueError):
        pcm.cluster_stats(Xt, lt, k, q=list(q), groups=torch.from_numpy(groups).cuda(), n_groups=257)


# ---------------------------------------------------------------- 6. additivity
def test_additivity_over_calls(pcm):
    n, k, G = 30_001, 16, 3
    X = blobs(n, 3, 11)
    labels = R.assign(X, X[R.init_indices(n, k)])
    groups = (np.arange(n) * G // n).astype(np.uint8)                  # one cloud per day, in row order
    q = list(R.fixed_q(X))
    want, _ = SR.encode(X, labels, k, q, groups, G)
    Xt, lt, gt = torch.from_numpy(X).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(groups).cuda()
    whole = pcm.cluster_stats(Xt, lt, k, groups=gt, n_groups=G)
    same(whole.numpy().view(np.uint64), want, "one call")
    h = 12_345
    part = pcm.cluster_stats(Xt[:h], lt[:h], k, groups=gt[:h], n_groups=G, q=q)
    back = pcm.cluster_stats(Xt[h:], lt[h:], k, groups=gt[h:], n_groups=G, q=q, out=part)
    assert back is part
    same(part.numpy().view(np.uint64), want, "two calls through out=")
    # one call per day, then + and merged
    days = [pcm.cluster_stats(Xt[gt == g], lt[gt == g], k, q=q) for g in range(G)]
    assert all(s.n_groups == 1 for s in days)
    same((days[0] + days[1] + days[2]).numpy().view(np.uint64), SR.encode(X, labels, k, q)[0], "sum of days")
    same(whole.merged().numpy().view(np.uint64), SR.encode(X, labels, k, q)[0], "merged")
    for g in range(G):
        same(days[g].numpy().view(np.uint64), want[g:g + 1], f"day {g}")
    with pytest.raises(ValueError):
        pcm.cluster_stats(Xt, lt, k, groups=gt, n_groups=G, q=[v + 1 for v in q], out=part)


def test_256_groups(pcm):
    n, k, G = 40_000, 4, 256
    X = blobs(n, 3, 12)
    rng = np.random.default_rng(12)
    labels = rng.integers(0, k, n).astype(np.int32)
    groups = np.sort(rng.integers(0, G, n))
    q = R.fixed_q(X)
    want, _ = SR.encode(X, labels, k, q, groups, G)
    assert (want[255, :, 0] > 0).any()
    got, sk, _ = raw(X, labels, k, q, groups, G)
    assert sk == 0
    same(got, want, "G = 256")
    st = pcm.cluster_stats(torch.from_numpy(X).cuda(), torch.from_numpy(labels).cuda(), k,
                           groups=torch.from_numpy(groups).cuda())      # n_groups = max + 1
    assert st.n_groups == 256
    same(st.numpy().view(np.uint64), want, "G = 256 wrapper")


# ---------------------------------------------------------------- 7. link to the engine
def test_means_are_the_fitted_centres(pcm):
    n, k = 20_000, 16
    X = blobs(n, 3, 21)
    Xt = torch.from_numpy(X).cuda()
    res = pcm.lloyd_fit(Xt, torch.from_numpy(X[R.init_indices(n, k)]).cuda(), max_iter=300, tol=0.0)
    assert res.strict
    st = pcm.cluster_stats(Xt, res.labels, k)
    labels = res.labels.cpu().numpy()
    assert np.array_equal(st.counts()[0], np.bincount(labels, minlength=k))
    got = st.means()[0].astype(np.float32)
    want = res.centers.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    same(st.numpy().view(np.uint64), SR.encode(X, labels, k, R.fixed_q(X))[0], "fit labels")


# ---------------------------------------------------------------- 8. plugin end to end
def test_plugin_describe_end_to_end(pcm):
    rng = np.random.default_rng(31)
    clouds = []
    for day in range(3):
        yy, xx = np.mgrid[0:70, 0:90]
        keep = rng.random(yy.shape) > 0.2
        if day == 2:
            keep &= xx < 45
        z = 6 * np.sin(xx / 19.0) + 4 * np.cos(yy / 13.0) + rng.normal(0, 0.2, yy.shape) + 0.5 * day
        clouds.append(np.stack([z[keep], yy[keep].astype(np.float64), xx[keep].astype(np.float64)], axis=1))
    dev = [torch.from_numpy(c).cuda() for c in clouds]
    k = 24
    layers, res = pcm.kmeans_fuse(clouds, n_clusters=k, describe=True, device_clouds=dev)
    X = np.concatenate(clouds).astype(np.float32)
    q = R.fixed_q(X)
    sizes = [c.shape[0] for c in clouds]
    groups = np.repeat(np.arange(3), sizes)
    want, _ = SR.encode(X, res["labels"], k, q, groups, 3)
    same(res["stats"]["words"].view(np.uint64), want, "kmeans_fuse describe")
    assert res["stats"]["q"] == list(q) and res["stats"]["sizes"] == sizes
    props = layers[0][1]["properties"]
    np.testing.assert_array_equal(props["count"], want[..., 0].sum(0).astype(np.int64))
    np.testing.assert_array_equal(props["days_seen"], (want[..., 0] > 0).sum(0))
    assert props["days_seen"].min() >= 2 and props["days_seen"].max() == 3
    assert np.isfinite(props["roughness"]).all() and (props["normal_z"] >= 0).all()
    zq = want.view(np.int64)[..., 1].astype(np.float64) * 2.0 ** -int(q[0])
    for j in range(k):
        mz = [zq[g, j] / float(want[g, j, 0]) for g in range(3) if want[g, j, 0]]
        assert props["height_spread"][j] == pytest.approx(max(mz) - min(mz), rel=1e-12, abs=1e-12)
    assert np.median(props["height_spread"][props["days_seen"] == 3]) > 0.5      # the days sit 0.5 apart
    # host clouds (no device_clouds) give the same words
    _, res_h = pcm.kmeans_fuse(clouds, n_clusters=k, describe=True)
    same(res_h["stats"]["words"].view(np.uint64), want, "host clouds")
    # a later day against the model
    later = [clouds[2] + np.array([0.25, 0.0, 0.0])]
    l2, r2 = pcm.kmeans_assign(later, res, describe=True)
    assert [l[1]["name"] for l in l2] == ["[Multi-day 3D Point Cloud] Assigned 3D Point Cloud",
                                          "[Multi-day 3D Point Cloud] Surface Change"]
    X2 = later[0].astype(np.float32)
    w2, _ = SR.encode(X2, r2["labels"], k, R.fixed_q(X2))
    same(r2["stats"]["words"].view(np.uint64), w2, "kmeans_assign describe")
    p2 = l2[1][1]["properties"]
    np.testing.assert_array_equal(p2["count"], np.bincount(r2["labels"], minlength=k))
    assert (p2["dz"][p2["count"] == 0] == 0).all() and (p2["count"] == 0).any()
    # without describe nothing changes
    l0, r0 = pcm.kmeans_assign(later, res)
    assert len(l0) == 1 and set(r0) == {"labels", "distance", "inertia", "n_points"}
