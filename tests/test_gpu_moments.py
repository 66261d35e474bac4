"""GPU: ``local_moments``, ``point_normals`` and the plugin's ``change_plane=``.  The ten words of every
row are compared bit for bit with the Python-integer brute force (tests/moments_ref.py): whichever
cells, runs and chunks the kernel walks, integer sums have one answer.  The planes are compared with
``np.linalg.eigh`` of the exact covariance within bounds that follow from float64 rounding alone
(DESIGN.md §4 "Local moments").
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import moments_ref as M  # noqa: E402
import nearest_ref as N  # noqa: E402
import support_ref as S  # noqa: E402

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


_brute = {}


def brute(name, X, Y, r, q):
    """The reference words of a named case, computed once."""
    key = (name, float(r), tuple(q))
    if key not in _brute:
        words, skipped, skipped_t = M.brute(X, Y, r, q)
        _brute[key] = (M.as_int64(words), skipped, skipped_t, words)
    return _brute[key]


def check(pcm, X, Y, r, q=None, name=None):
    """The kernel against the brute force (``Y is X``: one cloud, ``targets=None``) -> (LocalMoments, the words)."""
    Xd = dev(X, np.float32)
    lm = pcm.local_moments(Xd, r, targets=None if Y is X else dev(Y, np.float32), q=q)
    torch.cuda.synchronize()
    assert lm.q == (M.default_q(X, Y, r) if q is None else tuple(q))
    want = brute(name, X, Y, r, lm.q) if name else (M.as_int64(M.brute(X, Y, r, lm.q)[0]),)
    got = lm.words.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == (len(X), 10) and np.array_equal(got, want[0])
    finx, finy = np.isfinite(X).all(axis=1), np.isfinite(Y).all(axis=1)
    assert (lm.skipped, lm.skipped_targets) == (int((~finx).sum()), int((~finy).sum()))
    assert lm.radius == float(np.float32(r)) and torch.equal(lm.counts(), lm.words[:, 0])
    return lm, want[0]


# ---------------------------------------------------------------- 1. one cloud
@pytest.mark.parametrize("r", (0.75, 1.25, 2.5))
def test_one_cloud_on_the_lattice(pcm, r):
    X = S.lattice_cloud()
    lm, want = check(pcm, X, X, r, name="lattice")
    assert lm.cell_log2 == S.plan(X, r)[0] and 0.03 < (want[:, 0] > 1).mean()
    counts = pcm.radius_support(dev(X), r).counts
    assert torch.equal(lm.counts(), counts.to(torch.int64) + 1)       # support's neighbours and the row itself
    Xd = dev(X)
    same = pcm.local_moments(Xd, r, targets=Xd)                       # the same tensor: the one-cloud path
    other = pcm.local_moments(Xd, r, targets=Xd.clone())              # its copy: the two-cloud path
    assert torch.equal(same.words, lm.words) and torch.equal(other.words, lm.words)


# ---------------------------------------------------------------- 2. two clouds
@pytest.mark.parametrize("r, s", ((0.74, 0), (1.48, 1)))
def test_two_clouds_of_general_floats(pcm, r, s):
    X, Y = N.general_clouds()
    lm, want = check(pcm, X, Y, r)
    assert lm.cell_log2 == s and 0.05 < (want[:, 0] > 0).mean() < 0.95


def test_two_lattice_clouds(pcm):
    X, Y = N.lattice_clouds()
    lm, want = check(pcm, X, Y, 1.25, name="lattice pair")
    assert lm.cell_log2 == N.plan(X, Y, 1.25)[0] and (want[:, 0] > 0).any()


# ---------------------------------------------------------------- 3. faces
@pytest.mark.parametrize("r", (0.5, 1.0, 1.25, 3.0))
def test_faces(pcm, r):
    F = N.face_cloud(r)
    perm = np.random.default_rng(31).permutation(F.shape[0])
    lm, want = check(pcm, F, F[perm], r)
    assert (want[:, 0] >= 2).all() and lm.cell_log2 == N.radius_exponent(r)   # itself and its partner at exactly r


# ---------------------------------------------------------------- 4. crowded runs
@pytest.mark.parametrize("extra", (-1, 0, 1, None))
def test_crowded_runs(pcm, extra):
    from pcm_amd import _lib
    chunk = _lib.MOMENTS_CHUNK
    c = 3 * chunk + 5 if extra is None else chunk + extra
    X, Y, point = N.crowded_clouds(c)
    lm, want = check(pcm, X, Y, 1.0)
    assert want[0, 0] >= c and (want[1:, 0] >= 1).all()               # the duplicates add nothing but their count
    check(pcm, Y, Y, 1.0)                                             # and as queries: every one of them counts c


# ---------------------------------------------------------------- 5. wave and block edges, empty and non-finite
def test_sizes_and_nonfinite_rows(pcm):
    rng = np.random.default_rng(1)
    Y = (rng.random((300, 3)) * 3.0).astype(np.float32)
    for n in (1, 63, 64, 65, 257):
        check(pcm, (rng.random((n, 3)) * 3.0).astype(np.float32), Y, 0.8)
    X = (rng.random((65, 3)) * 3.0).astype(np.float32)
    for A, B in ((X, Y[:0]), (X[:0], Y), (X[:0], Y[:0])):
        lm, want = check(pcm, A, B, 0.8)
        assert lm.words.shape == (A.shape[0], 10) and not want.any()
    assert pcm.local_moments(dev(X[:0]), 0.8).words.shape == (0, 10)
    X, Y = X.copy(), Y.copy()
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        for a in range(3):
            X[3 * k + a, a] = v
            Y[(3 * k + a) * 7, a] = v
    lm, want = check(pcm, X, Y, 0.8)
    assert (lm.skipped, lm.skipped_targets) == (9, 9) and not want[:9].any() and want[9:, 0].sum() > 100
    lm, want = check(pcm, X, X, 0.8)                                  # one cloud: the skipped targets are the skipped queries
    assert (lm.skipped, lm.skipped_targets) == (9, 9) and (want[9:, 0] >= 1).all()
    nan = np.full((70, 3), np.nan, dtype=np.float32)
    for A, B in ((nan, Y), (X, nan), (nan, nan)):
        assert not check(pcm, A, B, 1.0)[1].any()


# ---------------------------------------------------------------- 6. row order
def test_row_order(pcm):
    X, Y = N.general_clouds()
    q = M.default_q(X, Y, 1.48)
    w0 = pcm.local_moments(dev(X), 1.48, targets=dev(Y), q=q).words
    px, py = np.random.default_rng(14).permutation(4096), np.random.default_rng(15).permutation(3000)
    w1 = pcm.local_moments(dev(X[px]), 1.48, targets=dev(Y), q=q).words
    w2 = pcm.local_moments(dev(X), 1.48, targets=dev(Y[py]), q=q).words
    assert torch.equal(w1, w0[dev(px)]) and torch.equal(w2, w0)
    assert torch.equal(pcm.local_moments(dev(X), 1.48, targets=dev(Y), q=q).words, w0)      # two calls


# ---------------------------------------------------------------- 7. words above 2^53
def test_words_above_2_53(pcm):
    from pcm_amd import moments
    X = M.clump_cloud()
    q = (24, 23, 23)
    assert X.shape == (2200, 3) and 2200 * M.bound(2.5, 24) ** 2 <= 1 << 62
    base = X[:2000]
    assert moments.check_q(q, M.maxabs(base, base), 2200, np.float32(2.5)) == q
    lm, want = check(pcm, X, X, 2.5, q=q, name="clumps")
    assert int(want.max()) > 1 << 53 and (want[2000:, 9] >= 100 * int(2.39 * 2 ** 23) ** 2).all()
    assert (want[2000:, 9] > 1 << 55).all() and (want[2000:, 0] == 200).all()     # beyond a float accumulator's 53 bits


# ---------------------------------------------------------------- 8. guards
def test_guards(pcm):
    X = np.concatenate(M.raster_days()[0])
    Xd = dev(X)
    with pytest.raises(ValueError, match="q"):
        pcm.local_moments(Xd, 1.6, q=(30, 30, 30))
    with pytest.raises(ValueError, match="q"):
        pcm.point_normals(Xd, 1.6, q=(30, 30, 30))
    with pytest.raises(ValueError, match="q"):
        pcm.local_moments(Xd, 1.6, q=(20, 19, 24))                    # |x| 2^24 reaches 2^31
    lm = pcm.local_moments(Xd, 1.6)
    assert lm.q == M.default_q(X, X, 1.6) == (20, 19, 17)
    Y = X[:500] * np.float32(8.0)
    assert pcm.local_moments(Xd, 1.6, targets=dev(Y)).q == M.default_q(X, Y, 1.6) != lm.q          # the box of both
    from pcm_amd import _lib
    with pytest.raises(_lib.PcmError, match="no CPU fallback"):
        pcm.local_moments(Xd, 1.6, targets=Xd.cpu())
    for bad in (Xd.double(), Xd[:, :2], Xd.reshape(-1)):
        with pytest.raises(ValueError, match="float32"):
            pcm.local_moments(bad, 1.6)
        with pytest.raises(ValueError, match="float32"):
            pcm.local_moments(Xd, 1.6, targets=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30, 1e-30, "x"):
        with pytest.raises(ValueError, match="radius"):
            pcm.local_moments(Xd, bad)


# ---------------------------------------------------------------- 9. planes
def plane_cases():
    raster = np.concatenate(M.raster_days()[0])
    lat = S.lattice_cloud()
    A, B = N.lattice_clouds()
    return {"raster 1.6": (raster, raster, 1.6), "raster 2.5": (raster, raster, 2.5), "lattice 1.25": (lat, lat, 1.25),
            "lattice 2.5": (lat, lat, 2.5), "lattice pair 2.5": (A, B, 2.5)}                # the last: two clouds, targets=


_planes = {}


def reference_planes(case):
    """(X, Y, r, q, words, planes at min_count 3) of a named case, computed once."""
    if case not in _planes:
        X, Y, r = plane_cases()[case]
        q = M.default_q(X, Y, r)
        words = brute(case.rsplit(" ", 1)[0], X, Y, r, q)           # the name the word tests use: shared with them
        _planes[case] = (X, Y, r, q, words, M.planes(words[3], q, 3))
    return _planes[case]


@pytest.mark.parametrize("case", ("raster 1.6", "raster 2.5", "lattice 1.25", "lattice 2.5", "lattice pair 2.5"))
def test_planes(pcm, case):
    X, Y, r, q, words, ref = reference_planes(case)
    Xd = dev(X)
    Yd = None if Y is X else dev(Y)
    lm = pcm.local_moments(Xd, r, targets=Yd)
    assert lm.q == q and np.array_equal(lm.words.cpu().numpy(), words[0])
    pn = pcm.point_normals(Xd, r, targets=Yd, moments=lm)
    torch.cuda.synchronize()
    count = words[0][:, 0]
    valid = count >= 3
    assert np.array_equal(pn.valid().cpu().numpy(), valid) and torch.equal(pn.count, lm.counts()) and 0 < valid.sum()
    normal, dist = pn.normal.cpu().numpy(), pn.distance.cpu().numpy()
    rough, planar = pn.roughness.cpu().numpy(), pn.planarity.cpu().numpy()
    assert normal.dtype == dist.dtype == rough.dtype == planar.dtype == np.float32 and normal.shape == (len(X), 3)
    for out in (normal[:, 0], normal[:, 1], normal[:, 2], dist, rough, planar):               # NaN exactly where not valid
        assert np.array_equal(np.isnan(out), ~valid)
    R = np.array([M.bound(r, q[a]) * 2.0 ** -q[a] for a in range(3)])
    Rm = R.max()
    # the float64 views: 9 roundings of at most 2^-53 R_a R_b each, bounded with margin
    cov = lm.covariances().cpu().numpy()
    err = np.abs(cov - ref["cov"])[count >= 1]
    print(f"{case}: cov error / (2^-52 R_a R_b) max {(err / (2.0 ** -52 * np.outer(R, R))).max():.3f}")
    assert cov.dtype == np.float64 and (err <= 32 * 2.0 ** -52 * np.outer(R, R)).all()
    assert np.isnan(cov[count < 1]).all()
    mu = lm.offsets().cpu().numpy()
    assert (np.abs(mu - ref["mu"])[count >= 1] <= 8 * 2.0 ** -52 * R).all()
    # the eigen-derived outputs
    lam = ref["lam"]
    e_r = np.abs(rough - ref["roughness"])[valid]
    print(f"{case}: roughness error max {e_r.max():.3e} (bound {2.0 ** -20 * Rm:.3e})")
    assert (e_r <= 2.0 ** -20 * Rm + 2.0 ** -23 * ref["roughness"][valid]).all()
    wide = valid & (lam[:, 2] >= 2.0 ** -10 * Rm * Rm)
    e_p = np.abs(planar - ref["planarity"])[wide]
    print(f"{case}: planarity error max {e_p.max():.3e} on {wide.sum()} rows")
    assert (e_p <= 2.0 ** -22).all() and (planar[valid & ~wide & (lam[:, 2] <= 0)] == 0).all()
    gap = valid & (lam[:, 1] - lam[:, 0] >= 2.0 ** -10 * Rm * Rm)
    share = gap.sum() / valid.sum()
    e_n = np.abs(normal - ref["normal"])[gap]
    e_d = np.abs(dist - ref["distance"])[gap]
    print(f"{case}: {gap.sum()} gap rows of {valid.sum()} valid ({share * 100:.2f} %), normal error max {e_n.max():.3e}, "
          f"distance error max {e_d.max():.3e} (bound {2.0 ** -21 * Rm:.3e})")
    assert share >= 0.95
    assert (e_n <= 2.0 ** -22).all() and (e_d <= 2.0 ** -21 * Rm).all()
    nv = normal[valid]
    assert (nv[:, 0] >= 0).all() and np.abs((nv.astype(np.float64) ** 2).sum(1) - 1).max() < 1e-6
    # min_count moves the NaN set; 0 means 1
    for k in (1, 5, 0):
        pk = pcm.point_normals(Xd, r, targets=Yd, min_count=k, moments=lm)
        assert np.array_equal(np.isnan(pk.roughness.cpu().numpy()), count < max(k, 1))
        assert np.array_equal(pk.valid().cpu().numpy(), count >= max(k, 1))
        both = count >= max(k, 3)
        assert np.array_equal(pk.normal.cpu().numpy()[both], normal[both])
    assert (count < 1).sum() <= (count < 3).sum() <= (count < 5).sum() and (count < 1).sum() < (count < 5).sum()
    fresh = pcm.point_normals(Xd, r, targets=Yd)                       # without moments=: the same call
    assert torch.equal(fresh.normal[dev(valid)], pn.normal[dev(valid)]) and torch.equal(fresh.count, pn.count)


# ---------------------------------------------------------------- 10. the plugin
def test_kmeans_assign_with_change_plane_on_the_device_path(pcm):
    from pcm_amd import plugin
    clouds, _ = M.raster_days(h=30, w=80)
    early, late = clouds[0].astype(np.float64), clouds[1].astype(np.float64) + np.array([0.5, 0.0, 0.0])
    _, model = plugin.kmeans_fuse([early], n_clusters=32, max_iter=10)
    layers, res = plugin.kmeans_assign([late], model, change=0.8, change_plane=3.0, change_to=early)
    X32, Y32 = late.astype(np.float32), early.astype(np.float32)
    pn = pcm.point_normals(dev(X32), 3.0, targets=dev(Y32))
    count = pn.count.cpu().numpy()
    few = count < 3
    props = layers[0][1]["properties"]
    want_d = np.where(few, np.nan, pn.distance.cpu().numpy().astype(np.float64))
    want_z = np.where(few, np.nan, pn.normal.cpu().numpy()[:, 0].astype(np.float64))
    assert np.array_equal(props["change_normal"], want_d, equal_nan=True)
    assert np.array_equal(props["change_normal_z"], want_z, equal_nan=True)
    cp = res["change_plane"]
    assert np.array_equal(cp["count"], count) and cp["radius"] == float(np.float32(3.0)) and 0 < few.sum() < few.size // 4
    assert np.array_equal(cp["distance"], want_d, equal_nan=True) and "change" in res and "change_dz" in props
    q = M.default_q(X32, Y32, 3.0)
    assert np.array_equal(count, M.as_int64(M.brute(X32, Y32, 3.0, q)[0])[:, 0])
    med = float(np.median(want_d[~few]))
    print(f"median change_normal {med:.4f} over {(~few).sum()} rows")
    assert abs(med - 0.5) <= 0.1                                      # noise 0.2 over about 11 neighbours
