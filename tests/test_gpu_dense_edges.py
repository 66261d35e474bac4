"""GPU: the edges of the dense engine (csrc/pcm_dense.hip) that the mid-range
shapes of tests/test_dense.py and section 9 of tests/test_gpu_predict.py never
reach: the LDS boundaries, the grid-stride loops, d = 1 and d = 64, relocation
in every branch, the histories, and the numeric edges of the fixed-point sums.

Every case equals ``oracle/dense_ref.py`` bit for bit (labels, centres, n_iter,
inertia, changed, shift, strict, relocations); seeding equals
``oracle/kpp_ref.py``.  ``test_fit_wide_precision`` is the one check that does
not share the oracle's arithmetic: labels against the argmin in the next-wider
float type (``wide_labels``), centres against the exact mean of their members
(``wide_centres``).

Unless a case says otherwise, X = normal(0, 1) * uniform(0.1, 5) per column
from ``default_rng(n + d + k)``, C0 = X[:k], max_iter = 8, tol = 0.
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import dense_ref as DR  # noqa: E402
from oracle import kpp_ref as P  # noqa: E402
from test_dense import RELOC_COUNT, reloc_case  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def pcm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pcm_amd
    from pcm_amd import _lib
    _lib.load()
    return pcm_amd


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def cloud(n, d, k, dtype):
    rng = np.random.default_rng(n + d + k)
    return (rng.normal(0, 1, (n, d)) * rng.uniform(0.1, 5, d)).astype(dtype)


def plain(n, d, k, dtype, max_iter=8):
    X = cloud(n, d, k, dtype)
    return X, X[:k].copy(), max_iter


def stride_cloud(dtype):
    """More rows than the assign grid covers in one round (4 * CU blocks of 256)."""
    return plain(1024 * cus() + 300, 2, 3, dtype, max_iter=4)


def columns(dtype):
    n, d, k = 4096, 5, 6
    X = cloud(n, d, k, dtype)
    X[:, 1] = 0.0                       # max |x| = 0: e_a = 0
    X[:, 2] = -8.0                      # a constant column, max |x| an exact power of two
    X[:, 3] = np.clip(X[:, 3], -4.0, 4.0)
    X[77, 3] = 4.0                      # max |x| = 2^2 exactly and n = 2^12: q_a = 62 - 3 - 13
    assert np.abs(X[:, 3]).max() == 4.0
    return X, X[:k].copy(), 8


def constant(dtype):
    X = np.full((4096, 2), -8.0, dtype)     # the sum is -2^60: the largest the bound allows at this n
    return X, X[:1].copy(), 8


def subnormal():
    """The 600 x 8, k = 6 cloud of test_gpu_dense_fit_random scaled by 2^-66 (exact):
    squared distances near 2^-132, below float32's smallest normal 2^-126."""
    rng = np.random.default_rng(600 + 8)
    X = (rng.normal(0, 1, (600, 8)) * rng.uniform(0.1, 5, 8)).astype(F32)
    X = np.ldexp(X, -66).astype(F32)
    return X, X[:6].copy(), 60


def ring_ties(dtype):
    """Distance ties among DISTINCT farthest rows: 700 rows on the 12 lattice points at
    squared distance exactly 25 from the only populated centre (0, 0), after 300 inner
    rows, and 5 empty clusters.  (distance desc, row asc) takes the five lowest ring rows,
    which sit in different threads of k_dense_update's scan and in its second and later
    rounds; any other tied rows are other points and give other centres.  (With identical
    tied rows, relocation case (c), the choice cannot be seen; scikit-learn's argpartition
    leaves it open, so this case is pinned to the oracle's rule only.)"""
    rng = np.random.default_rng(25)
    ring = np.array([(3, 4), (4, 3), (-3, 4), (-4, 3), (3, -4), (4, -3), (-3, -4), (-4, -3), (5, 0), (-5, 0), (0, 5),
                     (0, -5)], np.float64)
    inner = np.clip(rng.normal(0, 1, (300, 2)), -3, 3)
    X = np.concatenate([inner, ring[rng.integers(0, 12, 700)]]).astype(dtype)
    C0 = np.concatenate([[[0.0, 0.0]], np.full((5, 2), 900.0) + np.arange(5)[:, None]]).astype(dtype)
    return X, C0, 8


def relocation(name, dtype):
    return lambda: reloc_case(name, dtype)


# name -> (builder, centre check of wide_check applies)
FIT = {
    # dense_lds_c, k * d * sizeof(T) <= 64 KB: exactly 65 536 B of dynamic LDS (the largest legal
    # request), and one centre more (centres read from global memory; float32 only here)
    "ldsc-f64-k128": (lambda: plain(700, 64, 128, F64), True),
    "ldsc-f64-k129": (lambda: plain(700, 64, 129, F64), True),
    "ldsc-f32-k256": (lambda: plain(700, 64, 256, F32), True),
    "ldsc-f32-k257": (lambda: plain(700, 64, 257, F32), True),
    # dense_lds, centres + statistics <= 64 KB: the last k with both in LDS (65 520 B and
    # 65 504 B), and the first with the centres in LDS and the statistics in global memory
    "ldss-f64-k546": (lambda: plain(1200, 7, 546, F64), True),
    "ldss-f64-k547": (lambda: plain(1200, 7, 547, F64), True),
    "ldss-f32-k712": (lambda: plain(1500, 7, 712, F32), True),
    "ldss-f32-k713": (lambda: plain(1500, 7, 713, F32), True),
    # k_dense_assign's i += gridDim.x * blockDim.x, and the LDS statistics flush after
    # several rounds per thread
    "stride-f32": (lambda: stride_cloud(F32), True),
    "stride-f64": (lambda: stride_cloud(F64), True),
    # d = 1: dense_dist without its loop, shift with no full group of 4
    "d1-f32": (lambda: plain(2000, 1, 9, F32), True),
    "d1-f64": (lambda: plain(2000, 1, 9, F64), True),
    # k == n: every row its own centre; in float32 shift 0 stops the fit (done == 2) in iteration 1
    "keqn-f32": (lambda: plain(50, 5, 50, F32), True),
    "keqn-f64": (lambda: plain(50, 5, 50, F64), True),
    # max_iter = 1: stopped by the cap (done == 3) with one history entry
    "maxiter1-f32": (lambda: plain(3000, 7, 40, F32, max_iter=1), True),
    "maxiter1-f64": (lambda: plain(3000, 7, 40, F64, max_iter=1), True),
    # k_dense_update relocation (tests/test_dense.py::reloc_case): (a) three empty clusters;
    # (b) a donor emptied by the move copies the largest cluster; (c) ties among the farthest
    # rows across the 256-thread tree and more empty clusters than one pass fills; (d) every
    # row on its centre: the early break, no move.  In (b) the last iteration moves a row, so
    # a centre is then not the mean of any set of labels: no centre check there.
    "reloc-a-f64": (relocation("a", F64), True), "reloc-a-f32": (relocation("a", F32), True),
    "reloc-b1-f64": (relocation("b1", F64), False), "reloc-b1-f32": (relocation("b1", F32), False),
    "reloc-b2-f64": (relocation("b2", F64), False), "reloc-b2-f32": (relocation("b2", F32), False),
    "reloc-c-f64": (relocation("c", F64), True), "reloc-c-f32": (relocation("c", F32), True),
    "reloc-d-f64": (relocation("d", F64), True), "reloc-d-f32": (relocation("d", F32), True),
    # the tie rule v == bv && i < bi of the relocation scan, where the tied rows differ
    "ties-f64": (lambda: ring_ties(F64), True), "ties-f32": (lambda: ring_ties(F32), True),
    # q_a = 62 - e_a - bits(n): an all-zero column, a constant one, max |x| = 2^2 with n = 2^12
    "columns-f32": (lambda: columns(F32), True), "columns-f64": (lambda: columns(F64), True),
    # one cluster of 4096 rows of -8.0: |sum| = 2^60 in fixed point, the centre exactly -8.0
    "constant-f32": (lambda: constant(F32), True), "constant-f64": (lambda: constant(F64), True),
    # float32 distances that are subnormal (the unit keeps float32 denormals)
    "subnormal-f32": (subnormal, True),
}

_RUNS = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def gpu_fit(pcm, X, C0, max_iter, **kw):
    res = pcm.dense_fit(torch.from_numpy(X).cuda(), torch.from_numpy(C0).cuda(), max_iter=max_iter, tol=0.0,
                        **kw)
    torch.cuda.synchronize()
    return res


def run(pcm, name):
    """Oracle and GPU fit of one case, computed once for the tests that share it."""
    if name not in _RUNS:
        X, C0, max_iter = FIT[name][0]()
        ref = DR.dense_fit(X, C0, max_iter=max_iter, tol=0.0)
        _RUNS[name] = (X, C0, max_iter, ref, gpu_fit(pcm, X, C0, max_iter))
    return _RUNS[name]


def assert_equals_oracle(res, ref, where=""):
    labels, centers = res.labels.cpu().numpy(), res.centers.cpu().numpy()
    print(f"{where} n_iter={res.n_iter}/{ref['n_iter']} inertia={res.inertia!r}/{ref['inertia']!r} "
          f"relocations={res.relocations}/{ref['relocations']} strict={res.strict}/{ref['strict']}")
    bad = np.flatnonzero(labels != ref["labels"])
    assert labels.dtype == np.int32 and bad.size == 0, f"{where} {bad.size} labels differ, first rows {bad[:8]}"
    assert centers.dtype == ref["centers"].dtype
    bad = np.argwhere(bits(centers) != bits(ref["centers"]))
    assert bad.size == 0, f"{where} {len(bad)} centre entries differ, first {bad[:4].tolist()}"
    assert res.n_iter == ref["n_iter"], where
    assert res.inertia == ref["inertia"], where
    assert res.strict == ref["strict"], where
    assert res.relocations == ref["relocations"], where
    np.testing.assert_array_equal(res.changed, np.asarray(ref["changed"], np.int64), err_msg=where)
    np.testing.assert_array_equal(bits(res.shift), bits(np.asarray(ref["shift"], np.float64)), err_msg=where)


# ---------------------------------------------------------------- 1. fit against the oracle
@pytest.mark.parametrize("name", list(FIT))
def test_fit_equals_oracle(pcm, name):
    X, C0, max_iter, ref, res = run(pcm, name)
    assert_equals_oracle(res, ref, name)
    centers = res.centers.cpu().numpy()
    if name.startswith("reloc-"):
        case = name.split("-")[1]
        assert res.relocations == RELOC_COUNT[case]
        if case == "d":         # the still-empty clusters sit on the first largest cluster's centre
            assert res.relocations == 0
            np.testing.assert_array_equal(centers[3:], centers[[0, 0]])
            np.testing.assert_array_equal(np.bincount(res.labels.cpu().numpy(), minlength=5), [50, 50, 50, 0, 0])
        if case == "b1":        # the emptied donor (cluster 2) copied the largest cluster (1)
            np.testing.assert_array_equal(centers[2], centers[1])
    if name.startswith("ties-"):
        first = DR.dense_fit(X, C0, max_iter=1, tol=0.0)
        assert first["relocations"] == 1 and res.relocations >= 1
        np.testing.assert_array_equal(first["centers"][1:], X[300:305])     # the five lowest ring rows
        assert len(np.unique(X[300:305], axis=0)) > 1
    if name.startswith("constant-"):
        assert np.all(centers == -8.0) and res.n_iter == 1 and res.inertia == 0.0
    if name == "keqn-f32":      # (float64 rows lose low bits to the truncation at q_a: one more iteration)
        assert res.n_iter == 1 and not res.strict and res.shift[0] == 0.0 and res.changed[0] == 50
    if name.startswith("maxiter1-"):
        assert res.n_iter == 1 and not res.strict and len(res.changed) == 1 and len(res.shift) == 1
    if name == "subnormal-f32":
        sq = DR.assign(X, centers)[1]
        tiny = np.float32(np.finfo(np.float32).tiny)
        assert np.count_nonzero((sq > 0) & (sq < tiny)) > 0.5 * np.count_nonzero(sq > 0)
        assert np.bincount(ref["labels"], minlength=6).min() > 0 and ref["n_iter"] < 60


def test_fit_chunking(pcm):
    """chunk = 1 (a status read after every iteration) and chunk = 50 (longer than the
    fit: the launches after ``done`` are gated off) give the oracle's result and histories."""
    X, C0, _ = plain(600, 8, 6, F32)
    ref = DR.dense_fit(X, C0, max_iter=60, tol=0.0)
    assert 1 < ref["n_iter"] < 50
    one = gpu_fit(pcm, X, C0, 60, chunk=1)
    long = gpu_fit(pcm, X, C0, 60, chunk=50)
    assert_equals_oracle(one, ref, "chunk=1")
    assert_equals_oracle(long, ref, "chunk=50")
    assert torch.equal(one.labels, long.labels) and torch.equal(one.centers, long.centers)


# ---------------------------------------------------------------- 2. a check outside the oracle's arithmetic
def wide_type(dtype):
    return np.float64 if dtype == np.float32 else np.longdouble


def wide_labels(X, C, labels, where=""):
    """The label is the argmin in the next-wider type W on every row whose two smallest
    W distances differ by more than 2 (d + 2) eps_T relative to the larger: the rounding
    bound of two sequential d-term sums in T.  Rows under it are left out, at most 1 %
    of them (asserted first).  Bit-identical centres (a still-empty cluster copies the
    largest one) count as one centre, which the label must name by its lowest index."""
    n, d = X.shape
    W = wide_type(X.dtype)
    idx = np.unique(C, axis=0, return_index=True)[1]      # the lowest index of every distinct centre
    U = C[idx].astype(W)
    thr = W(2 * (d + 2)) * W(np.finfo(X.dtype).eps)
    left_out = wrong = 0
    step = max(1, (1 << 18) // max(1, len(U) * d))
    for s in range(0, n, step):
        D = ((X[s:s + step, None, :].astype(W) - U[None, :, :]) ** 2).sum(axis=2)
        a = np.argmin(D, axis=1)
        if len(U) > 1:
            two = np.partition(D, 1, axis=1)[:, :2]
            sure = (two[:, 1] - two[:, 0]) > thr * two[:, 1]
        else:
            sure = np.ones(len(D), bool)
        left_out += int(np.count_nonzero(~sure))
        wrong += int(np.count_nonzero(sure & (idx[a] != labels[s:s + step])))
    print(f"{where} wide labels: {left_out} of {n} rows left out, {wrong} differ")
    assert left_out <= 0.01 * n, f"{where} {left_out} of {n} rows are near-ties"
    assert wrong == 0, f"{where} {wrong} labels differ from the {np.dtype(W).name} argmin"


def wide_centres(X, C, members, where=""):
    """|c_ja - mean(members)_a| <= 2^-q_a + (3 eps_64 + eps_T / 2) |mean|: one truncation
    unit per row, averaged; the float64 roundings of the sum, of 1 / count and of their
    product (half an eps_64 each; the other half of the 3 covers the mean computed here: an
    exact sum, math.fsum, rounded once and divided once); the final rounding to T."""
    n, d = X.shape
    q = DR.fixed_q(np.abs(X).max(axis=0).astype(np.float64), n)
    rel = 3 * np.finfo(np.float64).eps + np.finfo(X.dtype).eps / 2
    worst = 0.0
    for j in np.unique(members):
        rows = X[members == j].astype(np.float64)
        for a in range(d):
            mean = math.fsum(rows[:, a]) / len(rows)
            bound = 2.0 ** -int(q[a]) + rel * abs(mean)
            err = abs(float(C[j, a]) - mean)
            worst = max(worst, err / bound)
            assert err <= bound, f"{where} centre {j} feature {a}: |{C[j, a]!r} - {mean!r}| = {err!r} > {bound!r}"
    print(f"{where} wide centres: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("name", list(FIT))
def test_fit_wide_precision(pcm, name):
    X, C0, max_iter, ref, res = run(pcm, name)
    if X.dtype == np.float64 and not np.finfo(np.longdouble).eps < 2.0 ** -60:
        pytest.skip("no float type wider than float64 here")
    labels, centers = res.labels.cpu().numpy(), res.centers.cpu().numpy()
    wide_labels(X, centers, labels, name)
    if not FIT[name][1]:
        return
    # the centres are the means of the labels of the last iteration's E-step: the final
    # labels after a strict stop; otherwise the labels against the centres one iteration
    # earlier, which a fit capped there returns (checked the same way first)
    if res.strict:
        members = labels
    elif res.n_iter == 1:
        members = pcm.dense_predict(torch.from_numpy(X).cuda(), torch.from_numpy(C0).cuda()).labels.cpu().numpy()
        wide_labels(X, C0, members, name + " (E-step of C0)")
    else:
        prev = gpu_fit(pcm, X, C0, res.n_iter - 1)
        members = prev.labels.cpu().numpy()
        wide_labels(X, prev.centers.cpu().numpy(), members, name + " (one iteration earlier)")
    wide_centres(X, centers, members, name)


# ---------------------------------------------------------------- 3. predict and transform
@pytest.mark.parametrize("dtype", [F32, F64])
def test_transform_grid_stride(pcm, dtype):
    """k_dense_transform's r0 += gridDim.x * rows: k = 2100 gives one row per chunk, and
    n = 4 CU + 37 rows are more than the 4 CU blocks of the grid."""
    n, d, k = 4 * cus() + 37, 3, 2100
    rng = np.random.default_rng(n + d + k)
    X = cloud(n, d, k, dtype)
    C = (X[rng.integers(0, n, k)] + rng.normal(0, 0.5, (k, d))).astype(dtype)
    T = pcm.dense_transform(torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()).cpu().numpy()
    want = np.sqrt(DR.sqdist(X, C))
    assert T.dtype == dtype and T.shape == (n, k)
    bad = np.flatnonzero(T != want)
    assert bad.size == 0, f"{bad.size} of {T.size} distances differ from the correctly rounded sqrt"


@pytest.mark.parametrize("dtype", [F32, F64])
def test_predict_grid_stride(pcm, dtype):
    """dense_predict over more rows than one round of the grid: labels, distances and
    the inertia limbs accumulated over several rows per thread."""
    X, C0, _ = stride_cloud(dtype)
    C = (C0 * 1.5).astype(dtype)
    res = pcm.dense_predict(torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda(), return_distance=True,
                            return_inertia=True)
    labels, sq = DR.assign(X, C)
    np.testing.assert_array_equal(res.labels.cpu().numpy(), labels)
    gd = res.distance.cpu().numpy()
    assert gd.dtype == dtype and np.array_equal(bits(gd), bits(sq))
    assert res.inertia == DR.inertia_exact(sq, DR.inertia_scale(np.abs(np.vstack([X, C])).max(axis=0)))


def test_predict_float32_overflow(pcm):
    """float32 squared distances that overflow to inf: the strict '<' keeps label 0 on a
    row whose distances are all inf, and the inertia is inf through the overflow limb."""
    n, d, k = 500, 4, 7
    rng = np.random.default_rng(n + d + k)
    X = (rng.normal(0, 1, (n, d)) * 1e20).astype(F32)
    C = X[:k].copy()
    with np.errstate(over="ignore"):
        labels, sq = DR.assign(X, C)
        want = DR.inertia_exact(sq, DR.inertia_scale(np.abs(np.vstack([X, C])).max(axis=0)))
    share = np.count_nonzero(np.isinf(sq)) / n
    print(f"rows with every distance inf: {share:.3f}, label 0: {np.count_nonzero(labels == 0) / n:.3f}")
    assert share > 0.9 and np.all(labels[np.isinf(sq)] == 0) and want == math.inf
    res = pcm.dense_predict(torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda(), return_distance=True,
                            return_inertia=True)
    np.testing.assert_array_equal(res.labels.cpu().numpy(), labels)
    assert np.array_equal(bits(res.distance.cpu().numpy()), bits(sq))
    assert res.inertia == math.inf


# ---------------------------------------------------------------- 4. dense k-means++
def dup_rows(distinct, times, d, dtype, seed):
    rng = np.random.default_rng(seed)
    X = np.repeat(rng.normal(0, 1, (distinct, d)).astype(dtype), times, axis=0)
    return X[rng.permutation(len(X))]


def tail_heavy(d, k, dtype):
    """4 202 501 rows = 1027 pass blocks of 4096; the last 8000 rows (inside blocks 1024 to
    1026) spread 40 times wider, so most of the potential, and most targets, lie there."""
    X = cloud(4_202_501, d, k, dtype)
    X[-8000:] *= 40
    return X


KPP = {  # name -> (X builder, k, n_local_trials)
    # k_dkpp_select with nblk = 1027 > 1024 pass blocks: two blocks per thread (per > 1)
    "blocks1027-f32-d2": (lambda: tail_heavy(2, 5, F32), 5, None),
    "blocks1027-f64-d1": (lambda: tail_heavy(1, 3, F64), 3, None),
    # duplicates: rows of weight zero inside the cumulative sum (side='left' skips them)
    "dup-k16": (lambda: dup_rows(400, 25, 5, F64, 16), 16, None),
    "dup-k40": (lambda: dup_rows(400, 25, 5, F32, 40), 40, None),
    # more centres than distinct rows: the potential reaches zero, every target is 0
    "dup-zero-potential": (lambda: dup_rows(3, 50, 4, F32, 5), 5, None),
    "k-equals-n": (lambda: cloud(300, 6, 300, F64), 300, None),
    "n1": (lambda: cloud(1, 3, 1, F32), 1, None),
    "d64": (lambda: cloud(3000, 64, 12, F32), 12, None),
    "d1": (lambda: cloud(3000, 1, 12, F32), 12, None),
    # n_local_trials at both ends of 1..DKPP_LMAX
    "trials1": (lambda: cloud(5000, 6, 10, F64), 10, 1),
    "trials16": (lambda: cloud(5000, 6, 10, F32), 10, 16),
}


@pytest.mark.parametrize("name", list(KPP))
def test_kmeanspp_equals_oracle(pcm, name):
    build, k, trials = KPP[name]
    X = build()
    seed = 7 + len(name)
    Cr, ir = P.kmeanspp(X, k, seed, n_local_trials=trials, keep_dtype=True)
    Cg, ig = pcm.dense_kmeanspp(torch.from_numpy(X).cuda(), k, random_state=seed, n_local_trials=trials)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ig.cpu().numpy(), ir)
    assert np.array_equal(bits(Cg.cpu().numpy()), bits(Cr))
