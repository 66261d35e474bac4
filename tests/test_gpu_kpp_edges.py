"""k-means++ seeding on the GPU at its edges: thin clouds (the grid clamp), every
trial count and kernel instantiation, branch coverage shown by the CPU
restatement (tests/kpp_geometry.py), crafted random streams that put targets at
the ends of the search, zero potentials, scale extremes and input handling.

Every case compares ``pcm_amd.kmeans_plusplus`` with ``oracle.kpp_ref.kmeanspp``:
equal indices, centres bitwise ``X[idx]``.  The chain checks itself: a wrong
weight, potential or block sum moves the later targets ``floor(u * pot)`` and
with them the chosen rows.
"""
import numpy as np
import pytest

import kpp_geometry as KG
from oracle import kpp_ref as P
from oracle import lloyd_ref as R


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pcm_amd
    return torch, pcm_amd


def _state(seed):
    """An int seed, or a zero-argument factory of a fresh RandomState per side."""
    return seed() if callable(seed) else seed


def same_as_oracle(gpu, X, k, seed, L=None, ref=None):
    torch, pcm = gpu
    i_ref = P.kmeanspp(X, k, _state(seed), L)[1] if ref is None else ref
    c, i = pcm.kmeans_plusplus(torch.from_numpy(X).cuda(), k, random_state=_state(seed), n_local_trials=L)
    assert i.dtype == torch.int64 and c.dtype == torch.float32
    i, c = i.cpu().numpy(), c.cpu().numpy()
    np.testing.assert_array_equal(i, i_ref)
    np.testing.assert_array_equal(c.view(np.uint32), X[i_ref].view(np.uint32))      # bitwise X[idx]
    return i_ref


def uniform(n, d, seed):
    return R.splitmix_uniform(n, d, seed=seed)


def clustered(n, d, seed=7):
    """12 clusters of sigma 0.05 in [-100, 100]^d."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-100, 100, size=(12, d))
    return (centres[rng.integers(0, 12, n)] + rng.normal(0, 0.05, (n, d))).astype(np.float32)


def thin_heightmap(n=150_000, seed=9):
    """Integer-pixel (z, y, x) cloud with two pixels of relief over an 1800 x 2400 image."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 1800, n).astype(np.float64)
    x = rng.integers(0, 2400, n).astype(np.float64)
    z = np.clip(0.6 * np.sin(x / 200) + 0.3 * np.cos(y / 150) + rng.normal(0, 0.05, n), -1.0, 1.0)
    return np.stack([z, y, x], axis=1).astype(np.float32)


# ---------------------------------------------------------------- thin clouds
def _thin_uniform(n, ext, seed):
    X = (uniform(n, len(ext), seed) * np.asarray(ext, np.float32)).astype(np.float32)
    assert (X.max(axis=0) > X.min(axis=0)).all()                    # no axis is constant
    return X


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,ext", KG.THIN, ids=[f"n{n}-k{k}-d{len(e)}" for n, k, e in KG.THIN])
def test_thin_clouds_of_predict(gpu, n, k, ext):
    X = _thin_uniform(n, ext, n + len(ext))
    assert KG.kpp_grid(X, clamp=False).ncells > KG.kpp_cells_max(n, len(ext))     # the clamp runs
    same_as_oracle(gpu, X, min(k, n), seed=n % 97)


@pytest.mark.gpu
def test_thin_heightmap(gpu):
    X = thin_heightmap()
    ext = X.max(axis=0) - X.min(axis=0)
    assert 0 < ext[0] <= 2 and ext[1] == 1799 and ext[2] == 2399
    g0, g = KG.kpp_grid(X, clamp=False), KG.kpp_grid(X)
    assert g0.ncells > KG.kpp_cells_max(len(X), 3) >= g.ncells and g.G[0] == 1
    same_as_oracle(gpu, X, 96, seed=21)


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,ext,seed", [(10_800, 16, (1, 90, 120), 3), (20_000, 24, (1, 1, 1e-5, 1), 8)],
                         ids=["1x90x120", "d4"])
def test_thin_small(gpu, n, k, ext, seed):
    X = _thin_uniform(n, ext, seed + 40)
    assert KG.kpp_grid(X, clamp=False).ncells > KG.kpp_cells_max(n, len(ext))
    same_as_oracle(gpu, X, k, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [False, True], ids=["constant", "few-ulp"])
def test_constant_axis(gpu, noise):
    """An exactly constant axis is left out of the grid's volume; with a few ulp of
    noise it is the thinnest axis a cloud can have."""
    n = 50_001
    X = uniform(n, 3, 3)
    X[:, 1] = np.float32(2.5)
    if noise:
        X[:, 1] += np.random.default_rng(1).integers(-2, 3, n).astype(np.float32) * np.float32(2.0 ** -22)
        assert np.unique(X[:, 1]).size == 5
        assert KG.kpp_grid(X, clamp=False).ncells > KG.kpp_cells_max(n, 3)
    else:
        assert KG.kpp_grid(X, clamp=False).ncells <= KG.kpp_cells_max(n, 3)
    assert (X.max(axis=0) > X.min(axis=0)).tolist() == [True, noise, True]
    same_as_oracle(gpu, X, 32, seed=13)


@pytest.mark.gpu
def test_thin_heightmap_seeding_then_fit(gpu):
    """The plugin's sequence on the thin height map: k-means++ centres, then Lloyd iterations."""
    from test_gpu_parity import assert_same, gpu_fit
    torch, pcm = gpu
    X = thin_heightmap(seed=10)
    i_ref = same_as_oracle(gpu, X, 96, seed=5)
    C0 = X[i_ref].copy()
    ref = R.lloyd_fit(X, C0, max_iter=5, fast=True)
    assert_same(gpu_fit(pcm, X, C0, 5), ref, "thin heightmap")


# ---------------------------------------------------------------- trial counts
@pytest.fixture(scope="module")
def cube20k():
    return uniform(20_000, 3, 55)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 8, 9, 16])
def test_trial_counts(gpu, cube20k, L):
    """k_kpp_eval<D, 8> up to 8 trials, the 16-accumulator instantiation from 9 on."""
    same_as_oracle(gpu, cube20k, 40, seed=L, L=L)


@pytest.mark.gpu
def test_sixteen_trials_d4(gpu):
    same_as_oracle(gpu, uniform(30_000, 4, 66), 24, seed=6, L=16)


@pytest.mark.gpu
def test_default_trials_reach_nine(gpu):
    assert P.n_trials(1096) == 8 and P.n_trials(1100) == 9
    same_as_oracle(gpu, uniform(4000, 3, 77), 1100, seed=2)


@pytest.mark.gpu
def test_trial_count_out_of_range(gpu, cube20k):
    """Both are raised before any launch: no index tensor comes back."""
    torch, pcm = gpu
    from pcm_amd._lib import PcmError
    Xt = torch.from_numpy(cube20k).cuda()
    with pytest.raises(ValueError, match="n_local_trials"):
        pcm.kmeans_plusplus(Xt, 12, random_state=0, n_local_trials=0)
    with pytest.raises(PcmError, match="n_local_trials must be 1..16"):
        pcm.kmeans_plusplus(Xt, 12, random_state=0, n_local_trials=17)


# ---------------------------------------------------------------- branches, shown by the restatement
# id, cloud, k, n_local_trials, the branches this cloud is here for (each: >= 5 steps).
# Trailing comments: step_branches' counts at seed 7, early/late eval steps, dense/sparse
# applies, late steps at c >= 64.  Up to 8 trials run k_kpp_eval<D, 8>, 9 to 16 the
# 16-accumulator instantiation: both have early and late steps, dense and sparse applies.
BRANCH = [
    ("clustered-d2-L16", lambda: clustered(80_000, 2), 40, 16, ("early", "late", "sparse")),         # 10/29, 1/37
    ("clustered-d3-L16", lambda: clustered(300_000, 3), 40, 16, ("early", "late")),                 # 11/28, 4/34
    ("clustered-d3-L9", lambda: clustered(120_000, 3), 40, 9, ("early", "late")),                   # 10/29, 4/34
    ("clustered-d3-L8", lambda: clustered(120_000, 3), 40, 8, ("early", "late", "dense", "sparse")),   # 11/28, 6/32
    ("uniform-d2-L9", lambda: uniform(200_000, 2, 31), 96, 9,
     ("early", "late", "late_at_c64", "sparse_at_c64")),                                            # 61/34, 1/93, 30
    ("uniform-d2-L6", lambda: uniform(200_000, 2, 31), 96, None, ("early", "late", "late_at_c64")),  # 36/59, 2/92, 32
    ("uniform-d1-L16", lambda: uniform(50_000, 1, 32), 80, 16, ("early", "late", "late_at_c64")),    # 30/49, 0/78, 16
    ("uniform-d3-L16", lambda: uniform(20_000, 3, 33), 40, 16, ("early", "dense")),                 # 39/0, 27/11
]
MIN_STEPS = 5


@pytest.mark.gpu
@pytest.mark.parametrize("name,cloud,k,L,named", BRANCH, ids=[b[0] for b in BRANCH])
def test_branches(gpu, name, cloud, k, L, named):
    X = cloud()
    idx, steps = KG.step_branches(X, k, 7, L)
    counts = KG.branch_counts(steps)
    print(name, counts)
    for b in named:
        assert counts[b] >= MIN_STEPS, (name, b, counts)
    i_ref = same_as_oracle(gpu, X, k, seed=7, L=L)
    np.testing.assert_array_equal(idx, i_ref)             # the restatement followed the oracle's steps


# ---------------------------------------------------------------- crafted random streams
EDGE_DRAWS = [0.0, 1.0 - 2.0 ** -53, 0.5, 0.25, 2.0 ** -53]


@pytest.mark.gpu
@pytest.mark.parametrize("first", [0.0, 1.0 - 2.0 ** -53], ids=["row0", "rowlast"])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193, 12_289])
def test_targets_at_the_ends(gpu, n, first):
    """Targets 0, pot - 1 and pot >> 53, the first centre on row 0 or n - 1, around the
    4096-row blocks of k_kpp_search (one row short, exact, one row into the next block)."""
    X = uniform(n, 3, n)
    idx = same_as_oracle(gpu, X, 6, seed=lambda: KG.CraftedState(first, EDGE_DRAWS), L=5)
    assert idx[0] == (0 if first == 0.0 else n - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("first", [0.0, 1.0 - 2.0 ** -53], ids=["row0", "rowlast"])
def test_targets_at_the_ends_rotating(gpu, first):
    """Four trials from a cycle of five: every step sees another part of the cycle."""
    X = uniform(9000, 3, 9)
    idx = same_as_oracle(gpu, X, 12, seed=lambda: KG.CraftedState(first, EDGE_DRAWS))
    assert idx[0] == (0 if first == 0.0 else 8999)


@pytest.mark.gpu
def test_random_state_is_consumed_as_sklearn_does(gpu):
    torch, pcm = gpu
    X = uniform(9000, 3, 10)
    rs_ref, rs_gpu = np.random.RandomState(11), np.random.RandomState(11)
    _, i_ref = P.kmeanspp(X, 12, rs_ref)
    _, i = pcm.kmeans_plusplus(torch.from_numpy(X).cuda(), 12, random_state=rs_gpu)
    np.testing.assert_array_equal(i.cpu().numpy(), i_ref)
    assert rs_gpu.random_sample() == rs_ref.random_sample()


# ---------------------------------------------------------------- zero potential, constant clouds
@pytest.mark.gpu
def test_more_centres_than_distinct_points(gpu):
    rng = np.random.default_rng(5)
    base = rng.uniform(-3, 3, (12, 3)).astype(np.float32)
    X = np.repeat(base, 400, axis=0)[rng.permutation(4800)]
    idx = same_as_oracle(gpu, X, 20, seed=3)
    assert len({X[i].tobytes() for i in idx[:12]}) == 12 and (idx[12:] == 0).all()


@pytest.mark.gpu
def test_one_repeated_point(gpu):
    X = np.tile(np.array([[1.5, -2.0, 3.25]], np.float32), (500, 1))
    idx = same_as_oracle(gpu, X, 5, seed=3)
    assert (idx[1:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 5])
def test_as_many_centres_as_points(gpu, n):
    idx = same_as_oracle(gpu, uniform(n, 3, n), n, seed=n)
    assert sorted(idx) == list(range(n))


# ---------------------------------------------------------------- scale
@pytest.mark.gpu
@pytest.mark.parametrize("e,scale", [(-30, 105), (40, -35)])
def test_power_of_two_scalings(gpu, cube20k, e, scale):
    """kpp_w with a large positive and a large negative shift.  A power-of-two scaling
    is exact, so the indices are also those of the unscaled cloud."""
    Xs = cube20k * np.float32(2.0 ** e)
    assert np.array_equal(Xs.astype(np.float64), cube20k.astype(np.float64) * 2.0 ** e)
    assert P.kpp_scale(len(Xs), P.max_dist_bound(Xs)) == scale
    # distances are multiples of 2**(2 * (e - 24)): far from fp32 subnormals
    i_ref = same_as_oracle(gpu, Xs, 24, seed=4)
    np.testing.assert_array_equal(i_ref, P.kmeanspp(cube20k, 24, 4)[1])


# ---------------------------------------------------------------- inputs
@pytest.mark.gpu
def test_half_input(gpu, cube20k):
    torch, pcm = gpu
    Xh = torch.from_numpy(cube20k).half()
    Xf = Xh.float().numpy()
    _, i_ref = P.kmeanspp(Xf, 16, 8)
    c, i = pcm.kmeans_plusplus(Xh.cuda(), 16, random_state=8)
    np.testing.assert_array_equal(i.cpu().numpy(), i_ref)
    np.testing.assert_array_equal(c.cpu().numpy(), Xf[i_ref])


@pytest.mark.gpu
def test_double_input(gpu, monkeypatch):
    """float64 points: distances on the float32 cast, the first draw against float64 unit weights."""
    torch, pcm = gpu
    n, u0 = 5000, 2501 / 5000          # a draw on a cdf step: the weights' dtype decides the first row
    assert (P.first_index(n, u0, np.float64), P.first_index(n, u0, np.float32)) == (2500, 2501)
    X = uniform(n, 3, 12)
    later = np.random.RandomState(1).random_sample(64)

    def seed():
        return KG.CraftedState(u0, later)

    first = P.first_index
    monkeypatch.setattr(P, "first_index", lambda m, u, dtype=None: first(m, u, np.float64))
    _, i_ref = P.kmeanspp(X, 16, seed())
    monkeypatch.undo()
    assert i_ref[0] == 2500
    c, i = pcm.kmeans_plusplus(torch.from_numpy(X).double().cuda(), 16, random_state=seed())
    np.testing.assert_array_equal(i.cpu().numpy(), i_ref)
    np.testing.assert_array_equal(c.cpu().numpy(), X[i_ref])


@pytest.mark.gpu
def test_strided_view(gpu):
    torch, pcm = gpu
    X4 = uniform(20_000, 4, 14)
    view = torch.from_numpy(X4).cuda()[:, :3]
    assert not view.is_contiguous()
    X = np.ascontiguousarray(X4[:, :3])
    _, i_ref = P.kmeanspp(X, 16, 9)
    c, i = pcm.kmeans_plusplus(view, 16, random_state=9)
    np.testing.assert_array_equal(i.cpu().numpy(), i_ref)
    np.testing.assert_array_equal(c.cpu().numpy(), X[i_ref])


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nonfinite_input(gpu, bad):
    torch, pcm = gpu
    X = uniform(5000, 3, 15)
    X[4321, 1] = bad
    with pytest.raises(ValueError, match="NaN or Inf"):
        pcm.kmeans_plusplus(torch.from_numpy(X).cuda(), 12, random_state=0)


@pytest.mark.gpu
def test_bad_arguments(gpu):
    torch, pcm = gpu
    from pcm_amd._lib import PcmError
    X = uniform(100, 3, 16)
    for k in (101, 0, -1):
        with pytest.raises(ValueError):
            pcm.kmeans_plusplus(torch.from_numpy(X).cuda(), k, random_state=0)
    with pytest.raises(PcmError):
        pcm.kmeans_plusplus(torch.from_numpy(X), 12, random_state=0)          # a CPU tensor: no fallback
