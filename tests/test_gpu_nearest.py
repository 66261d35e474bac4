"""GPU: ``nearest_points`` and the plugin's ``change=``, every output bitwise against the NumPy brute
force (tests/nearest_ref.py): whichever cells, runs and chunks the kernel walks, index and squared
distance are the same bits, and a tie in distance goes to the lowest target row.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import nearest_ref as N  # noqa: E402

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


def run(pcm, X, Y, r, gx=None, gy=None):
    Xd = dev(X, np.float32)
    Yd = Xd if Y is X else dev(Y, np.float32)
    near = pcm.nearest_points(Xd, Yd, r, groups=None if gx is None else dev(gx),
                              target_groups=None if gy is None else dev(gy))
    torch.cuda.synchronize()
    return near, near.index.cpu().numpy(), near.sqdist.cpu().numpy()


def check(pcm, X, Y, r, gx=None, gy=None, want=None):
    """The kernel against the brute force; -> (Nearest, the reference's tuple)."""
    want = want or N.brute(X, Y, r, gx, gy)
    near, index, sq = run(pcm, X, Y, r, gx, gy)
    assert index.dtype == np.int32 and index.shape == (len(X),) and np.array_equal(index, want[0])
    assert sq.dtype == np.float32 and np.array_equal(sq.view(np.uint32), want[1].view(np.uint32))
    assert (near.skipped, near.skipped_targets) == want[2:4] and near.max_dist == float(np.float32(r))
    assert np.array_equal(near.found().cpu().numpy(), want[0] >= 0)
    assert torch.equal(near.distance(), torch.sqrt(near.sqdist)) and near.distance().dtype == torch.float32
    return near, want


# ---------------------------------------------------------------- 1. general floats
@pytest.mark.parametrize("r, s", ((0.74, 0), (1.48, 1)))
def test_general_floats(pcm, r, s):
    X, Y = N.general_clouds()
    near, want = check(pcm, X, Y, r)
    share = (want[0] >= 0).mean()
    print(f"r={r}: {share * 100:.1f} % found, cell_log2 {near.cell_log2}")
    assert 0.05 < share < 0.95 and near.cell_log2 == s


# ---------------------------------------------------------------- 2. the exact-distance lattice
@pytest.fixture(scope="module")
def lattice():
    X, Y = N.lattice_clouds()
    return X, Y, np.random.default_rng(11).integers(0, 3, X.shape[0])


@pytest.mark.parametrize("r", (0.75, 1.25, 2.5))
def test_lattice(pcm, lattice, r):
    X, Y, days = lattice
    near, want = check(pcm, X, Y, r)
    assert 0.03 < (want[0] >= 0).mean() < 0.95 and near.cell_log2 == N.plan(X, Y, r)[0]
    assert (want[1] == np.float32(r) * np.float32(r)).any()           # pairs at exactly r


def test_lattice_other_day_and_other_row(pcm, lattice):
    X, _, days = lattice
    near, want = check(pcm, X, X, 1.25, days, days)                   # the nearest point of another day
    found = want[0] >= 0
    assert 0.05 < found.mean() < 0.95 and (days[want[0][found]] != days[found]).all()
    own = np.arange(X.shape[0])
    for r in (0.75, 1.25, 2.5):                                       # arange excludes the row itself:
        near, want = check(pcm, X, X, r, own, own)                    # found <=> radius_support counts a neighbour
        counts = pcm.radius_support(dev(X), r).counts
        assert torch.equal(near.found(), counts > 0) and 0 < int(near.found().sum()) < X.shape[0]


# ---------------------------------------------------------------- 3. ties
def test_ties_go_to_the_lowest_row(pcm):
    X, Y = N.tie_clouds()
    near, want = check(pcm, X, Y, 1.5)
    print(f"{(want[0] >= 0).sum()} found, {want[4]} tied, {(want[1] == 0).sum()} at distance 0")
    assert want[4] >= 300
    perm = np.random.default_rng(23).permutation(Y.shape[0])
    near2, want2 = check(pcm, X, Y[perm], 1.5)                        # the same points in other rows
    assert np.array_equal(want2[1], want[1]) and not np.array_equal(perm[want2[0]], want[0])


# ---------------------------------------------------------------- 4. faces
@pytest.mark.parametrize("r", (0.5, 1.0, 1.25, 3.0))
def test_faces(pcm, r):
    F = N.face_cloud(r)
    perm = np.random.default_rng(31).permutation(F.shape[0])
    near, want = check(pcm, F, F[perm], r, np.arange(F.shape[0]), perm)
    assert (want[1] == np.float32(r) * np.float32(r)).sum() >= 1 and (want[0] >= 0).all()
    assert near.cell_log2 == N.radius_exponent(r)


# ---------------------------------------------------------------- 5. crowded cells
@pytest.mark.parametrize("extra", (-1, 0, 1, None))
def test_crowded_cells(pcm, extra):
    from pcm_amd import _lib
    chunk = _lib.NEAREST_CHUNK
    c = 3 * chunk + 5 if extra is None else chunk + extra
    X, Y, point = N.crowded_clouds(c)
    near, want = check(pcm, X, Y, 1.0)
    copies = np.flatnonzero((Y == point).all(axis=1))
    assert copies.size == c and want[0][0] == copies.min() and want[1][0] == 0      # the lowest duplicate row wins
    assert (want[0][1:] >= 0).all()
    groups = np.arange(Y.shape[0]) % 4                                # with the group plane staged beside the records
    check(pcm, X, Y, 1.0, np.arange(X.shape[0]) % 4, groups)


# ---------------------------------------------------------------- 6. sizes
def test_sizes(pcm):
    from pcm_amd import _lib
    rng = np.random.default_rng(1)
    tpb = _lib.NEAREST_TPB
    sizes = (0, 1, 63, 64, 65, tpb - 1, tpb, tpb + 1)
    clouds = {k: (rng.random((k, 3)) * 3.0).astype(np.float32) for k in sizes}
    others = {k: (rng.random((k, 3)) * 3.0).astype(np.float32) for k in sizes}
    pairs = {(n, n) for n in sizes} | {(n, m) for n in sizes for m in (0, 1, 65, tpb + 1)} | \
        {(n, m) for n in (0, 1, 65, tpb + 1) for m in sizes}
    assert {(0, 0), (0, 65), (65, 0)} <= pairs
    for n, m in sorted(pairs):
        near, want = check(pcm, clouds[n], others[m], 0.8)
        assert near.index.shape == (n,) and near.sqdist.shape == (n,)
        if n and m:
            check(pcm, clouds[n], others[m], 0.8, np.arange(n) % 2, np.arange(m) % 2)
        if not m:
            assert (want[0] == -1).all() and np.isinf(want[1]).all()


# ---------------------------------------------------------------- 7. further inputs
def test_thin_clouds(pcm):
    rng = np.random.default_rng(6)
    flat = np.array([0.0, 30.0, 30.0]), np.array([2.5, 0.0, 0.0])
    X = (rng.random((1500, 3)) * flat[0] + flat[1]).astype(np.float32)
    Y = (rng.random((1200, 3)) * flat[0] + flat[1]).astype(np.float32)
    _, want = check(pcm, X, Y, 0.9)                                   # constant z
    assert 0.05 < (want[0] >= 0).mean()
    t, u = rng.random(1500).astype(np.float32) * 40, rng.random(900).astype(np.float32) * 40
    _, want = check(pcm, np.stack([t * 0.5, -t, t * 0.25], axis=1), np.stack([u * 0.5, -u, u * 0.25], axis=1), 0.1)
    assert 0.05 < (want[0] >= 0).mean()                               # all rows on a line
    P = np.tile(np.float32([1, 2, 3]), (200, 1))
    _, want = check(pcm, P, P.copy(), 0.1)                            # one point, 200 times on both sides
    assert (want[0] == 0).all() and (want[1] == 0).all()


def test_forced_coarsening(pcm):
    rng = np.random.default_rng(9)
    a = (rng.random((400, 3)) * 0.05).astype(np.float32)
    b = (rng.random((300, 3)) * 0.05).astype(np.float32)
    X = np.concatenate([a, a[::-1] + np.float32([0, 0, 1e6])]).astype(np.float32)
    Y = np.concatenate([b + np.float32([0, 0, 1e6]), b]).astype(np.float32)
    near, want = check(pcm, X, Y, 0.01)                               # two clumps 10^6 apart
    assert N.radius_exponent(0.01) == -6 and near.cell_log2 == N.plan(X, Y, 0.01)[0] > -6
    assert (want[0][:400] >= 300).any() and (want[0][400:] >= 0).any() and (want[0][400:] < 300).all()


def test_disjoint_and_outside(pcm):
    rng = np.random.default_rng(10)
    Y = (rng.random((800, 3)) * 4.0).astype(np.float32)
    X = (rng.random((500, 3)) * 4.0).astype(np.float32) + np.float32([0, 100, 0])
    _, want = check(pcm, X, Y, 1.0)                                   # disjoint boxes
    assert (want[0] == -1).all()
    shell = (rng.random((1200, 3)) * 7.0 - 1.5).astype(np.float32)    # queries around Y's box on every side
    outside = ((shell < 0) | (shell > 4)).any(axis=1)
    _, want = check(pcm, shell[outside], Y, 0.6)
    found = want[0] >= 0
    assert 20 < found.sum() < outside.sum()
    for a in range(3):
        assert (found & (shell[outside][:, a] < 0)).any() and (found & (shell[outside][:, a] > 4)).any()


# ---------------------------------------------------------------- 8. non-finite rows
def test_nonfinite_rows(pcm):
    rng = np.random.default_rng(13)
    Y = (rng.random((1000, 3)) * 6.0).astype(np.float32)
    X = Y[rng.permutation(1000)[:900]] + np.float32(0.01)             # every query has a target ...
    bad_y = rng.choice(1000, 90, replace=False)
    bad_x = rng.choice(900, 45, replace=False)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):                 # ... until one of the two is not a point
        for a in range(3):
            Y[bad_y[(3 * k + a) * 10:(3 * k + a + 1) * 10], a] = v
            X[bad_x[(3 * k + a) * 5:(3 * k + a + 1) * 5], a] = v
    near, want = check(pcm, X, Y, 0.5)
    assert (near.skipped, near.skipped_targets) == (45, 90)
    index, sq = near.index.cpu().numpy(), near.sqdist.cpu().numpy()
    assert (index[bad_x] == -1).all() and np.isinf(sq[bad_x]).all()
    assert not np.isin(index, bad_y).any() and (index >= 0).sum() > 700
    check(pcm, X, Y, 0.5, np.arange(900) % 3, np.arange(1000) % 3)
    nan = np.full((70, 3), np.nan, dtype=np.float32)
    near, want = check(pcm, nan, Y, 1.0)                              # no finite query at all
    assert near.skipped == 70 and (want[0] == -1).all()
    near, want = check(pcm, X, nan, 1.0)                              # no finite target at all
    assert near.skipped_targets == 70 and (want[0] == -1).all()
    check(pcm, nan, nan.copy(), 1.0)


# ---------------------------------------------------------------- 9. order
def test_order(pcm):
    X, Y = N.general_clouds()
    gx, gy = np.arange(4096) % 5 - 2, np.arange(3000) % 5 - 2
    _, i0, s0 = run(pcm, X, Y, 1.48, gx, gy)
    _, i1, s1 = run(pcm, X, Y, 1.48, gx, gy)
    assert np.array_equal(i0, i1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))      # two calls
    perm = np.random.default_rng(14).permutation(4096)
    _, i2, s2 = run(pcm, X[perm], Y, 1.48, gx[perm], gy)
    assert np.array_equal(i2, i0[perm]) and np.array_equal(s2.view(np.uint32), s0[perm].view(np.uint32))
    want = N.brute(X, Y, 1.48, gx, gy)
    assert np.array_equal(i0, want[0]) and np.array_equal(s0, want[1])
    # group values are compared for equality only: any int32 values, any integer dtype
    big = np.array([-2 ** 31, 2 ** 31 - 1, 0, 64, 1000], dtype=np.int64)
    _, i3, s3 = run(pcm, X, Y, 1.48, big[gx + 2], big[gy + 2])
    _, i4, _ = run(pcm, X, Y, 1.48, (gx + 2).astype(np.uint8), (gy + 2).astype(np.int16))
    assert np.array_equal(i3, i0) and np.array_equal(s3, s0) and np.array_equal(i4, i0)


# ---------------------------------------------------------------- 10. the Python errors
def test_python_errors(pcm):
    from pcm_amd import _lib
    X, Y = dev(np.zeros((10, 3), np.float32)), dev(np.ones((7, 3), np.float32))
    with pytest.raises(_lib.PcmError, match="no CPU fallback"):
        pcm.nearest_points(X.cpu(), Y, 1.0)
    with pytest.raises(_lib.PcmError, match="no CPU fallback"):
        pcm.nearest_points(X, Y.cpu(), 1.0)
    for bad in (X.double(), X[:, :2], X.reshape(-1)):
        with pytest.raises(ValueError, match="float32"):
            pcm.nearest_points(bad, Y, 1.0)
        with pytest.raises(ValueError, match="float32"):
            pcm.nearest_points(X, bad, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30, 1e39, 1e-30, "x"):
        with pytest.raises(ValueError, match="max_dist"):
            pcm.nearest_points(X, Y, bad)
    gx, gy = dev(np.arange(10)), dev(np.arange(7))
    with pytest.raises(ValueError, match="go together"):
        pcm.nearest_points(X, Y, 1.0, groups=gx)
    with pytest.raises(ValueError, match="go together"):
        pcm.nearest_points(X, Y, 1.0, target_groups=gy)
    for bad in (gx[:9], gx.float(), gx > 3, gx.cpu(), gx.reshape(2, 5)):
        with pytest.raises(ValueError, match="groups must be an integer device tensor"):
            pcm.nearest_points(X, Y, 1.0, groups=bad, target_groups=gy)
    for bad in (gy[:6], gy.double(), gy > 3):
        with pytest.raises(ValueError, match="target_groups must be an integer device tensor"):
            pcm.nearest_points(X, Y, 1.0, groups=gx, target_groups=bad)
    with pytest.raises(ValueError, match="int32 values"):
        pcm.nearest_points(X, Y, 1.0, groups=gx + (1 << 31), target_groups=gy)
    with pytest.raises(ValueError, match="int32 values"):
        pcm.nearest_points(X, Y, 1.0, groups=gx, target_groups=gy - (1 << 31) - 1)
    near = pcm.nearest_points(X, Y, 2.0, groups=gx, target_groups=gy)
    assert near.index.tolist() == [1] + [0] * 9 and near.sqdist.tolist() == [3.0] * 10      # row 0 skips its own group


# ---------------------------------------------------------------- 11. the plugin
def test_kmeans_assign_with_change_on_the_device_path(pcm):
    from pcm_amd import plugin
    rng = np.random.default_rng(15)
    yy, xx = np.meshgrid(np.arange(40.0), np.arange(60.0), indexing="ij")
    early = np.stack([3.0 * np.sin(xx / 23.0) + 2.0 * np.cos(yy / 7.0), yy, xx], axis=-1).reshape(-1, 3)
    late = early[rng.random(2400) < 0.6] + np.array([0.05, 0.3, -0.2])
    late[:200, 0] += 1.5                                               # change beyond max_dist
    _, model = plugin.kmeans_fuse([early], n_clusters=32, max_iter=10)
    layers, res = plugin.kmeans_assign([late], model, change=0.8, change_to=early)
    X32, Y32 = late.astype(np.float32), early.astype(np.float32)
    index, sq, *_ = N.brute(X32, Y32, 0.8)
    found = index >= 0
    assert 0 < (~found).sum() < found.size // 2
    want_dz = np.full(found.size, np.nan)
    want_dz[found] = X32[found, 0].astype(np.float64) - Y32[index[found], 0].astype(np.float64)
    props = layers[0][1]["properties"]
    assert np.array_equal(props["change"], np.where(found, np.sqrt(sq.astype(np.float64)), np.nan), equal_nan=True)
    assert np.array_equal(props["change_dz"], want_dz, equal_nan=True)
    assert np.array_equal(res["change"]["index"], index) and np.array_equal(res["change"]["found"], found)
