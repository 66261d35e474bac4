"""GPU: ``pcm_align_stats`` / ``pcm_align_apply`` and everything built on them, bitwise on all 38
words of every group plus the skipped word against the NumPy reference (tests/align_ref.py):
whichever path a row takes -- its cell's list, all K centres outside the grid's box, the provable
outlier shortcut, the carried wave sums or the per-lane atomics -- the words are the same bits.
"""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import align_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

N = 50_000


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


def default_q(X, C, T):
    from pcm_amd import align
    X = np.asarray(X, dtype=np.float32)
    fin = np.where(np.isfinite(X), np.abs(X), 0)
    return align.default_q(fin.max(0) if X.shape[0] else np.zeros(3), np.abs(C).max(0), T)


def raw(X, C, q, groups=None, G=1, T=None, max_dist=None, plan=None, buf=None):
    """pcm_align_stats itself: uint64 words (G, 38), the skipped word, the buffer and the plan."""
    from pcm_amd import _lib, align
    lib = _lib.load()
    n = X.shape[0]
    Xt = dev(X, np.float32)
    if plan is None:
        plan = align.AlignPlan(dev(C, np.float32), n, max_dist)
    gt = None if groups is None else dev(groups, np.uint8)
    Tt = None if T is None else dev(np.asarray(T, dtype=np.float32).reshape(-1, 12))
    if buf is None:
        buf = torch.zeros(G * A.WORDS + 1, dtype=torch.int64, device="cuda")
    qa = np.ascontiguousarray(q, dtype=np.int32)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = lib.pcm_align_stats(p(Xt) if n else None, n, p(gt) if n else None, G, p(Tt),
                             ctypes.c_float(align._max_d2(max_dist)), qa.ctypes.data_as(ctypes.c_void_p), p(buf), None,
                             p(plan.ws), ctypes.byref(plan.plan), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint64)
    return host[:-1].reshape(G, A.WORDS).copy(), int(host[-1]), buf, plan


def same(got, want, where=""):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and bad.size == 0, \
        f"{where}: {bad.shape[0]} words differ, first (g, w) {bad[:6].tolist()}: " \
        f"got {[hex(int(got[tuple(b)])) for b in bad[:3]]} want {[hex(int(want[tuple(b)])) for b in bad[:3]]}"


def check(X, C, groups=None, G=1, T=None, max_dist=None, where="", plan=None, q=None):
    """One GPU pass against ``encode``: all words and the skipped word.  -> (words, skipped, plan)."""
    from pcm_amd import align
    q = default_q(X, C, T) if q is None else q
    want, wskip = A.encode(X, C, q, groups, G, T, align._max_d2(max_dist))
    got, gskip, _, plan = raw(X, C, q, groups, G, T, max_dist, plan)
    same(got, want, where)
    assert gskip == wskip, (where, gskip, wskip)
    return got, gskip, plan


def blobs(n, seed, nb=12, sd=0.8, shift=-3.0):
    rng = np.random.default_rng(seed)
    centers = rng.random((nb, 3)) * 10 + shift
    return (centers[rng.integers(0, nb, n)] + rng.normal(0, sd, (n, 3))).astype(np.float32)


def rigid(rng, G, angle=0.03, shift=0.3):
    """Small random rigid motions, (G, 12) float32."""
    T = np.zeros((G, 12))
    for g in range(G):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        th = rng.uniform(-angle, angle)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        T[g, :9] = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)).ravel()
        T[g, 9:] = rng.uniform(-shift, shift, 3)
    return T.astype(np.float32)


def identity(G):
    return np.tile(np.r_[np.eye(3).ravel(), np.zeros(3)].astype(np.float32), (G, 1))


def run_order(key, lengths=(37, 64, 100), seed=3):
    """A row order whose runs of equal key have lengths cycling through ``lengths`` (they straddle the 64-row rounds)."""
    rng = np.random.default_rng(seed)
    pools = [list(np.flatnonzero(key == v)) for v in np.unique(key)]
    out, t = [], 0
    while any(pools):
        live = [p for p in pools if p]
        p = live[rng.integers(len(live))]
        L = lengths[t % len(lengths)]
        t += 1
        out += p[:L]
        del p[:L]
    return np.asarray(out)


# ---------------------------------------------------------------- orders and options
@pytest.mark.parametrize("K", [1, 16, 300])
@pytest.mark.parametrize("G", [1, 3])
def test_orders_and_options(pcm, K, G):
    rng = np.random.default_rng(10 * K + G)
    X = blobs(N, 5)
    C = X[np.sort(rng.choice(N, K, replace=False))] + np.float32(0.05)
    days = np.sort(rng.integers(0, G, N)).astype(np.uint8)                # days concatenated
    d2 = A.R.sqdist_rows(X, C[A.R.assign(X, C)])
    some = float(np.sqrt(np.median(d2)))                                  # leaves inliers and outliers
    orders = {"days": np.arange(N), "random": rng.permutation(N), "runs": run_order(days)}
    for tname, T in (("none", None), ("identity", identity(G)), ("rigid", rigid(rng, G))):
        for max_dist in (None, some):
            plan = None
            for oname, o in orders.items():
                grp = None if (G == 1 and oname == "days") else days[o]
                got, _, plan = check(X[o], C, grp, G, T, max_dist, f"K={K} G={G} T={tname} md={max_dist} {oname}", plan)
                if max_dist is not None:
                    assert got[:, 0].sum() > 0 and got[:, 1].sum() > 0
                else:
                    assert got[:, 0].sum() == N and got[:, 1].sum() == 0


# ---------------------------------------------------------------- sizes and grid
@pytest.mark.parametrize("blocks", [None, "1", "7"])
def test_sizes_and_grid(pcm, blocks, monkeypatch):
    if blocks is None:
        monkeypatch.delenv("PCM_ALIGN_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("PCM_ALIGN_BLOCKS", blocks)
    rng = np.random.default_rng(2)
    Xall = blobs(50_001, 6)
    C = Xall[np.sort(rng.choice(Xall.shape[0], 40, replace=False))]
    T = rigid(rng, 3)
    for n in (0, 1, 63, 64, 65, 257, 50_001):
        X = Xall[:n]
        groups = np.sort(rng.integers(0, 3, n)).astype(np.uint8)
        got, skipped, _ = check(X, C, groups, 3, T, 1.0, f"n={n} blocks={blocks}", q=default_q(Xall, C, T))
        assert int(got[:, :2].sum()) == n and skipped == 0


# ---------------------------------------------------------------- box paths
def test_unit_cube_centres_in_a_wide_cloud(pcm):
    """Most rows lie outside the inflated box: provable outliers with a finite max_dist, all-K scans with none."""
    rng = np.random.default_rng(4)
    C = rng.random((64, 3)).astype(np.float32)
    X = (rng.random((N, 3)) * 100 - 50).astype(np.float32)
    X[:2000] = (rng.random((2000, 3)) * 1.5 - 0.25).astype(np.float32)      # some in and around the cube
    X = X[rng.permutation(N)]
    groups = np.sort(rng.integers(0, 2, N)).astype(np.uint8)
    got, _, _ = check(X, C, groups, 2, None, 0.2, "finite")
    assert got[:, 0].sum() > 0 and got[:, 1].sum() > N // 2
    got, _, _ = check(X, C, groups, 2, rigid(rng, 2), None, "none")
    assert got[:, 0].sum() == N


def test_centres_far_outside_the_cloud(pcm):
    rng = np.random.default_rng(5)
    X = blobs(N, 7)
    C = (X[np.sort(rng.choice(N, 50, replace=False))] + np.float32(1000.0)).astype(np.float32)
    check(X, C, None, 1, None, None, "far, no trimming")
    some = float(np.sqrt(np.median(A.R.sqdist_rows(X, C[A.R.assign(X, C)]))))
    got, _, _ = check(X, C, None, 1, None, some, "far, trimmed")
    assert got[0, 0] > 0 and got[0, 1] > 0


def test_rows_at_the_faces_of_the_inflated_box(pcm):
    """Rows a few ulps on both sides of the grid box's faces (box of the centres inflated by
    sqrt(max_d2) (1 + 1e-6)) and of the provable-outlier bound (clo - r, chi + r)."""
    rng = np.random.default_rng(6)
    C = (rng.random((30, 3)) * 8 + 1).astype(np.float32)
    max_dist = 0.75
    m = np.float32(max_dist)
    pad = np.sqrt(np.float64(m * m)) * (1.0 + 1e-6)
    clo, chi = C.min(0), C.max(0)
    rows = []
    for a in range(3):
        for face in (np.float64(clo[a]) - pad, np.float64(chi[a]) + pad, np.float64(clo[a]) - np.float64(m),
                     np.float64(chi[a]) + np.float64(m), np.float64(clo[a]), np.float64(chi[a])):
            f = np.float32(face)
            for steps in range(-4, 5):
                v = f
                for _ in range(abs(steps)):
                    v = np.nextafter(v, np.float32(np.inf if steps > 0 else -np.inf))
                for base in C[rng.choice(30, 3)]:
                    r = base.copy()
                    r[a] = v
                    rows.append(r)
    X = np.asarray(rows, dtype=np.float32)
    got, _, _ = check(X, C, None, 1, None, max_dist, "faces")
    assert got[0, 0] > 0 and got[0, 1] > 0
    check(X, C, None, 1, None, None, "faces, no trimming")


def test_d2_equal_to_max_d2_is_an_inlier(pcm):
    C = np.array([[0, 0, 0], [100, 0, 0], [0, 100, 0], [0, 0, 100]], dtype=np.float32)
    X = np.array([[3, 4, 0], [100, 3, 4], [4, 100, 3],                         # d2 == 25 exactly
                  [3, np.nextafter(np.float32(4), np.float32(5)), 0], [0, 0, 94.5]], dtype=np.float32)   # just beyond
    got, _, _ = check(X, C, None, 1, None, 5.0, "d2 == max_d2")
    assert (got[0, 0], got[0, 1]) == (3, 2)


# ---------------------------------------------------------------- degenerate centres
def test_degenerate_centres(pcm):
    rng = np.random.default_rng(8)
    X = blobs(N, 9)
    groups = np.sort(rng.integers(0, 2, N)).astype(np.uint8)
    one = X[:1] + np.float32(0.5)
    check(X, one, groups, 2, None, None, "K = 1")
    check(X, one, groups, 2, None, 3.0, "K = 1 trimmed")
    check(X, np.repeat(one, 2, axis=0), groups, 2, None, None, "identical")
    check(X, np.repeat(one, 2, axis=0), groups, 2, None, 3.0, "identical trimmed")
    check(X, np.zeros((2, 3), dtype=np.float32), groups, 2, None, None, "identical at the origin")
    flat = X[np.sort(rng.choice(N, 40, replace=False))].copy()
    flat[:, 0] = np.float32(1.25)                                                # coplanar
    check(X, flat, groups, 2, None, None, "coplanar")
    check(X, flat, groups, 2, rigid(rng, 2), 1.0, "coplanar trimmed")
    line = flat.copy()
    line[:, 1] = np.float32(-2.0)                                                # collinear
    check(X, line, groups, 2, None, None, "collinear")


def test_crowded_centres_with_full_cells(pcm):
    rng = np.random.default_rng(11)
    n = 3000
    C = (rng.normal(0, 0.05, (4096, 3)) + 2.0).astype(np.float32)
    X = (rng.normal(0, 0.08, (n, 3)) + 2.0).astype(np.float32)
    got, _, plan = check(X, C, None, 1, None, None, "crowded")
    assert plan.info["full_cells"] > 0, plan.info
    check(X, C, None, 1, None, 0.01, "crowded trimmed", )


# ---------------------------------------------------------------- skips
def test_skipped_rows(pcm):
    from pcm_amd import align
    rng = np.random.default_rng(12)
    n = 5000
    X = blobs(n, 13)
    C = X[np.sort(rng.choice(n, 20, replace=False))]
    groups = np.sort(rng.integers(0, 3, n)).astype(np.uint8)
    q = default_q(X, C, None)
    clean, _ = A.encode(X, C, q, groups, 3)
    for name, edit in (("nan", lambda X, g: X.__setitem__((17, 1), np.nan)), ("inf", lambda X, g: X.__setitem__((90, 2), -np.inf)),
                       ("group", lambda X, g: g.__setitem__(4000, 3))):
        Xb, gb = X.copy(), groups.copy()
        edit(Xb, gb)
        got, skipped, _ = check(Xb, C, gb, 3, None, None, name, q=q)
        assert skipped == 1 and int(got[:, 0].sum()) == n - 1
        assert int((got != clean).any(1).sum()) == 1          # the other groups' rows are untouched
    # a transform that pushes group 1 past 2^QBITS of the exponents: every row of it is skipped, nothing else changes
    T = identity(3)
    T[1, 9] = np.float32(1e6)
    got, skipped, _ = check(X, C, groups, 3, T, None, "range", q=q)
    assert skipped == int((groups == 1).sum()) and not got[1].any()
    same(got[[0, 2]], clean[[0, 2]], "range: other groups")
    Xd, Cd, gd = dev(X), dev(C), dev(groups)
    with pytest.raises(ValueError, match="skipped"):
        align.align_stats(Xd, Cd, groups=gd, n_groups=3, transforms=T, q=q)
    Xb = X.copy()
    Xb[5, 0] = np.nan
    with pytest.raises(ValueError, match="skipped 1 rows"):
        align.align_stats(dev(Xb), Cd, groups=gd, n_groups=3)


# ---------------------------------------------------------------- additivity and fusion
def test_chunks_apply_and_fusion(pcm):
    from pcm_amd import align
    rng = np.random.default_rng(14)
    X = blobs(N, 15)
    C = X[np.sort(rng.choice(N, 100, replace=False))]
    groups = rng.integers(0, 3, N).astype(np.uint8)
    T = rigid(rng, 3)
    Xd, Cd, gd = dev(X), dev(C), dev(groups)
    plan = align.AlignPlan(Cd, N, 1.5)
    one = align.align_stats(Xd, Cd, groups=gd, n_groups=3, transforms=T, max_dist=1.5, plan=plan)
    want, skipped = A.encode(X, C, one.q, groups, 3, T, align._max_d2(1.5))
    same(one.numpy().view(np.uint64), want, "wrapper")
    acc = None
    for a, b in ((0, 17_001), (17_001, 17_064), (17_064, N)):
        acc = align.align_stats(Xd[a:b], Cd, groups=gd[a:b], n_groups=3, transforms=T, max_dist=1.5, q=one.q, out=acc,
                                plan=plan)
    same(acc.numpy().view(np.uint64), want, "three chunks")
    moved = align.apply_registration(Xd, T, gd)
    assert np.array_equal(moved.cpu().numpy().view(np.uint32), A.transform(X, T, groups).view(np.uint32))
    fused = align.align_stats(moved, Cd, groups=gd, n_groups=3, max_dist=1.5, q=one.q, plan=plan)
    same(fused.numpy().view(np.uint64), want, "apply then stats")


# ---------------------------------------------------------------- driver
def test_register_days_recovers_the_displacement(pcm):
    """``register_days`` on the recovery case: the same R, t and n_iter as ``align_ref.register`` (equal words,
    the same host code) and the recovery bounds of tests/test_align.py."""
    from pcm_amd import align
    case = A.recovery_case()
    ref, ref_error = A.recovery_reference()
    X1 = dev(case["X"][case["n0"]:])
    reg = align.register_days(X1, dev(case["C"]), kind="rigid")
    assert reg.n_iter == ref.n_iter and reg.n_iter <= 50
    assert np.array_equal(reg.R, ref.R) and np.array_equal(reg.t, ref.t)
    assert np.array_equal(reg.transforms, ref.transforms) and np.array_equal(reg.inliers, ref.inliers)
    assert np.array_equal(reg.rms_before, ref.rms_before) and np.array_equal(reg.rms_after, ref.rms_after)
    err = A.point_error(align.apply_registration(X1, reg).cpu().numpy(), case)
    print(f"displacement {case['rms0']:.3f} -> point error {err:.4f}; rms {reg.rms_before} -> {reg.rms_after}")
    assert err <= 0.31 and err == ref_error
    assert np.all(reg.rms_after <= reg.rms_before)


# ---------------------------------------------------------------- plugin
def test_plugin_fuse_with_registration_matches_the_stand_in(pcm):
    from pcm_amd import plugin
    clouds, ref_align = A.two_days(), A.ref_align
    gl, gr = plugin.kmeans_fuse(clouds, n_clusters=64, max_iter=20, register="rigid")
    wl, wr = plugin.kmeans_fuse(clouds, n_clusters=64, max_iter=20, register="rigid", align=ref_align)
    for key in ("R", "t", "transforms", "inliers", "outliers", "rms_before", "rms_after", "ok"):
        assert np.array_equal(gr["registration"][key], wr["registration"][key], equal_nan=key.startswith("rms")), key
    assert gr["registration"]["n_iter"] == wr["registration"]["n_iter"]
    assert np.array_equal(gl[1][0], wl[1][0])                     # the fused cloud: the registered points
    assert np.array_equal(gr["labels"], wr["labels"]) and np.array_equal(gr["centers"], wr["centers"])
