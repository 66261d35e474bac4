"""CPU: the registration ABI's argument checks, the ``AlignStats`` accessors and solves on words from
the NumPy reference (tests/align_ref.py), the driver on the recovery case, and the plugin's
``register=`` paths through the ``align=`` stand-in (the product has no CPU fallback; the HIP
kernels are checked in tests/test_gpu_align.py).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import align_ref as A
from oracle import lloyd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blobs(n, seed, nb=12, sd=0.8):
    rng = np.random.default_rng(seed)
    centers = rng.random((nb, 3)) * 10 - 3
    return (centers[rng.integers(0, nb, n)] + rng.normal(0, sd, (n, 3))).astype(np.float32)


def rotation(axis, angle):
    ax = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


# ---------------------------------------------------------------- ABI
def test_header_exports_and_abi_version():
    from pcm_amd import _lib
    src = open(os.path.join(ROOT, "include", "pcm_kmeans.h")).read()
    for name in ("pcm_align_workspace", "pcm_align_prepare", "pcm_align_stats", "pcm_align_apply"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTS
    assert re.search(r"#define\s+PCM_ALIGN_WORDS\s+38\b", src) and _lib.ALIGN_WORDS == 38 == A.WORDS
    assert re.search(r"#define\s+PCM_ALIGN_MAXG\s+256\b", src) and _lib.ALIGN_MAXG == 256
    assert re.search(r"#define\s+PCM_ABI_VERSION\s+8\b", src) and _lib.ABI_VERSION == 8
    assert any(u.endswith("pcm_align.hip") for u in _lib.UNITS)
    assert ctypes.sizeof(_lib.PcmAlignPlan) == 512


def test_argument_errors_without_device():
    """Every argument check of the four entry points runs before any device call."""
    from pcm_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    lib = _lib.load(require_gpu_runtime=False)
    one = ctypes.c_void_p(256)      # a non-null address that is never dereferenced
    nbytes = ctypes.c_size_t()
    assert lib.pcm_align_workspace(1000, 16, ctypes.byref(nbytes)) == 0 and nbytes.value > 16 * 32
    small = nbytes.value
    assert lib.pcm_align_workspace(1 << 24, 4096, ctypes.byref(nbytes)) == 0 and nbytes.value > small
    assert lib.pcm_align_workspace(1000, 0, ctypes.byref(nbytes)) == -1 and "k must be" in _lib.last_error()
    assert lib.pcm_align_workspace(-1, 4, ctypes.byref(nbytes)) == -1 and "n must be" in _lib.last_error()
    assert lib.pcm_align_workspace(10, 4, None) == -1
    plan = _lib.PcmAlignPlan()
    inf = ctypes.c_float(float("inf"))
    assert lib.pcm_align_prepare(None, 4, 10, inf, one, 1 << 30, ctypes.byref(plan), None, None) == -1
    assert lib.pcm_align_prepare(one, 4, 10, ctypes.c_float(-1.0), one, 1 << 30, ctypes.byref(plan), None, None) == -1
    assert "max_d2" in _lib.last_error()
    assert lib.pcm_align_prepare(one, 4, 10, ctypes.c_float(float("nan")), one, 1 << 30, ctypes.byref(plan), None, None) == -1
    assert lib.pcm_align_prepare(one, 4, 10, inf, one, 8, ctypes.byref(plan), None, None) == -1
    assert "workspace too small" in _lib.last_error()
    q = (ctypes.c_int32 * 3)(0, 0, 0)

    def stats(n=10, G=1, md=inf, qq=q, p=plan, X=one, out=one):
        return lib.pcm_align_stats(X, n, None, G, None, md, qq, out, None, one, ctypes.byref(p) if p else None, None)

    for kw, word in ((dict(n=-1), "n must be"), (dict(n=1 << 31), "2^31"), (dict(G=0), "n_groups"), (dict(G=257), "n_groups"),
                     (dict(md=ctypes.c_float(-2.0)), "max_d2"), (dict(qq=None), "null"), (dict(p=None), "null")):
        assert stats(**kw) == -1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert stats() == -3 and "not prepared" in _lib.last_error()      # PCM_E_STATE: a zeroed plan
    for kw in (dict(n=-1), dict(G=0), dict(G=257), dict(T=None), dict(X=None), dict(out=None)):
        a = dict(X=one, n=5, G=1, T=one, out=one)
        a.update(kw)
        assert lib.pcm_align_apply(a["X"], a["n"], None, a["G"], a["T"], a["out"], None) == -1, kw
    assert lib.pcm_align_apply(None, 0, None, 1, one, None, None) == 0


def test_public_names():
    import torch

    import pcm_amd
    for name in ("align_stats", "AlignStats", "register_days", "Registration", "apply_registration"):
        assert name in pcm_amd.__all__ and getattr(pcm_amd, name) is not None
    for call in (lambda: pcm_amd.align_stats(torch.zeros(4, 3), torch.zeros(2, 3)),
                 lambda: pcm_amd.register_days(torch.zeros(4, 3), torch.zeros(2, 3)),
                 lambda: pcm_amd.apply_registration(torch.zeros(4, 3), np.zeros((1, 12)))):
        with pytest.raises(pcm_amd._lib.PcmError):      # host tensors: no CPU fallback
            call()


# ---------------------------------------------------------------- encoder and accessors
@pytest.fixture(scope="module")
def small():
    """3000 points, K = 9, G = 3, a rigid motion per group and a trimming radius: small enough for Python ints."""
    from pcm_amd import align
    X = blobs(3000, 5)
    C = X[R.init_indices(3000, 9)] + np.float32(0.1)
    groups = np.random.default_rng(1).integers(0, 3, 3000).astype(np.uint8)
    T = np.stack([np.r_[rotation((1, 2, 3), 0.02 * (g + 1)).ravel(), [0.1 * g, -0.2, 0.3]] for g in range(3)]).astype(np.float32)
    q = align.default_q(np.abs(X).max(0), np.abs(C).max(0), T)
    max_d2 = align._max_d2(2.0)
    words, skipped = A.encode(X, C, q, groups, 3, T, max_d2)
    assert skipped == 0
    return X, C, groups, T, q, max_d2, words


def test_encoder_matches_python_int_sums(small):
    from pcm_amd import align
    X, C, groups, T, q, max_d2, words = small
    want, skipped = A.direct(X, C, q, groups, 3, T, max_d2)
    st = align.AlignStats(words, q)
    assert skipped == 0 and st.n_groups == 3
    assert st.inliers().tolist() == [r["inliers"] for r in want] and min(st.inliers()) > 0
    assert st.outliers().tolist() == [r["outliers"] for r in want] and min(st.outliers()) > 0
    assert int(st.inliers().sum() + st.outliers().sum()) == 3000
    assert st.sums_p().tolist() == [r["sp"] for r in want] and st.sums_c().tolist() == [r["sc"] for r in want]
    assert st.cross().tolist() == [r["cross"] for r in want]
    assert st.sq_p().tolist() == [r["sqp"] for r in want] and st.sq_c().tolist() == [r["sqc"] for r in want]
    assert st.numpy().dtype == np.int64 and st.numpy().shape == (3, 38)


def test_add_and_merged(small):
    from pcm_amd import align
    X, C, groups, T, q, max_d2, words = small
    a, _ = A.encode(X[:1700], C, q, groups[:1700], 3, T, max_d2)
    b, _ = A.encode(X[1700:], C, q, groups[1700:], 3, T, max_d2)
    both = align.AlignStats(a, q) + align.AlignStats(b, q)
    assert np.array_equal(both.numpy().view(np.uint64), words)
    one = align.AlignStats(words, q).merged()
    assert one.n_groups == 1 and np.array_equal(one.numpy().view(np.uint64)[0], words.sum(0, dtype=np.uint64))
    assert one.cross()[0].tolist() == align.AlignStats(words, q).cross().sum(0).tolist()
    with pytest.raises(ValueError):
        both + align.AlignStats(a, [v + 1 for v in q])
    with pytest.raises(ValueError):
        align.AlignStats(np.zeros((2, 37), dtype=np.int64), q)


def test_rms_is_the_rms_distance_of_the_inliers(small):
    from pcm_amd import align
    X, C, groups, T, q, max_d2, words = small
    g, valid, inl, pq, cq = A.rows(X, C, groups, 3, T, max_d2, q)
    scale = np.ldexp(1.0, -np.asarray(q, dtype=np.int64))
    d2 = (((pq - cq) * scale) ** 2).sum(1)
    want = np.array([np.sqrt(d2[inl & (g == k)].mean()) for k in range(3)])
    assert np.allclose(align.AlignStats(words, q).rms(), want, rtol=1e-12, atol=0)


# ---------------------------------------------------------------- solves
def exact_stats(P, Cm, q=(30, 30, 30), groups=None, G=1):
    """AlignStats of matched pairs (p_i, c_i) given in float64, formed in Python ints at the exponents ``q``
    (the words are an exact container: nothing in the accessors depends on QBITS)."""
    from pcm_amd import align
    words = np.zeros((G, 38), dtype=object)
    g = np.zeros(len(P), dtype=int) if groups is None else groups
    for i in range(len(P)):
        p = [int(np.trunc(np.ldexp(P[i, a], q[a]))) for a in range(3)]
        c = [int(np.trunc(np.ldexp(Cm[i, a], q[a]))) for a in range(3)]
        w = words[g[i]]
        w[0] += 1
        prods = [p[a] * c[b] for a in range(3) for b in range(3)] + [v * v for v in p] + [v * v for v in c]
        for a in range(3):
            w[2 + a] += p[a]
            w[5 + a] += c[a]
        for j, v in enumerate(prods):
            w[8 + 2 * j] += v & A.MASK
            w[9 + 2 * j] += v >> 32
    return align.AlignStats(np.array([[int(v) % (1 << 64) for v in row] for row in words], dtype=np.uint64), list(q))


def test_solve_recovers_known_motions():
    """Points on the 2^-10 lattice are exact at q = 30; their images under the motion are truncated at 2^-30,
    so the solves recover a z shift, a translation and a rigid motion to 1e-9 * the cloud's extent (8)."""
    rng = np.random.default_rng(3)
    P = np.round(rng.random((60, 3)) * 8 * 1024) / 1024
    for kind, Rt, tt in (("z", np.eye(3), np.array([0.75, 0.0, 0.0])),
                         ("translation", np.eye(3), np.array([-1.3, 1.7, -2.2])),
                         ("rigid", rotation((0.3, 1.0, 0.2), np.deg2rad(0.4)), np.array([-1.3, 1.7, -2.2])),
                         ("rigid", rotation((1.0, -2.0, 0.5), 1.1), np.array([3.0, -0.5, 0.25]))):
        st = exact_stats(P, P @ Rt.T + tt)
        Rs, ts, ok = st.solve(kind)
        assert ok.all() and np.abs(Rs[0] - Rt).max() <= 1e-9 and np.abs(ts[0] - tt).max() <= 8e-9, (kind, Rs, ts)
        assert st.rms()[0] == pytest.approx(np.sqrt((((P @ Rt.T + tt) - P) ** 2).sum(1).mean()), rel=1e-7)
    # a reflection is not a rigid motion: the solve returns a proper rotation
    st = exact_stats(P, P * np.array([1.0, 1.0, -1.0]))
    Rs, ts, ok = st.solve("rigid")
    assert np.linalg.det(Rs[0]) == pytest.approx(1.0, abs=1e-12)
    with pytest.raises(ValueError):
        st.solve("affine")


def test_degenerate_groups_fall_back():
    rng = np.random.default_rng(4)
    P = np.round(rng.random((40, 3)) * 8 * 1024) / 1024
    t = np.array([0.5, -0.25, 1.0])
    groups = np.r_[np.zeros(30, int), [1, 1], np.full(8, 3)]       # group 2 is empty
    Pg = P.copy()
    Pg[32:] = P[32] + np.outer(np.arange(8), [0.0, 1.0, 0.0])      # group 3: collinear (rank 1)
    st = exact_stats(Pg, Pg + t, groups=groups, G=4)
    Rs, ts, ok = st.solve("rigid")
    assert ok.tolist() == [True, False, False, False]
    for g in (1, 3):                                               # fewer than 3 inliers, rank below 2: translation
        assert np.array_equal(Rs[g], np.eye(3)) and np.abs(ts[g] - t).max() <= 1e-8
    assert np.array_equal(Rs[2], np.eye(3)) and np.array_equal(ts[2], np.zeros(3))      # no inliers: identity
    assert np.isnan(st.rms()[2])
    Rs, ts, ok = st.solve("translation")
    assert ok.tolist() == [True, True, False, True] and np.array_equal(ts[2], np.zeros(3))
    Rs, ts, ok = st.solve("z")
    assert np.abs(ts[[0, 1, 3]] - [0.5, 0, 0]).max() <= 1e-8 and np.array_equal(ts[2], np.zeros(3))


# ---------------------------------------------------------------- the driver
def test_recovery_of_a_displaced_day():
    """The issue's case: day 1 of the 240 x 240 terrain, displaced by 0.4 degrees about (0.3, 1, 0.2) and
    (-1.3, 1.7, -2.2) (rms 3.110), registered onto the K = 256 Lloyd centres of day 0 without trimming.
    ``align_ref.register`` reaches a point error of 0.0532 in 37 iterations; the day's rms to the model goes
    from 6.612 to 6.403.  Bounds: error <= 0.31, rms_after <= rms_before, n_iter <= 50."""
    case = A.recovery_case()
    reg, err = A.recovery_reference()
    print(f"displacement {case['rms0']:.4f} -> point error {err:.4f} in {reg.n_iter} iterations; "
          f"rms {reg.rms_before} -> {reg.rms_after}")
    assert case["rms0"] == pytest.approx(3.11, abs=0.005)
    assert err <= 0.31
    assert np.all(reg.rms_after <= reg.rms_before)
    assert reg.n_iter <= 50 and reg.converged and reg.ok.all()
    assert reg.inliers[0] == case["X"].shape[0] - case["n0"] and reg.outliers[0] == 0


def test_height_only_registration_converges_fast():
    case = A.recovery_case()
    X1 = case["true1"].astype(np.float32)[::8] + np.float32([2.5, 0, 0])
    reg = A.register(X1, case["C"], None, 1, kind="z")
    assert reg.n_iter <= 6 and reg.converged
    assert np.array_equal(reg.R[0], np.eye(3)) and reg.t[0, 1] == 0 and reg.t[0, 2] == 0
    assert abs(reg.t[0, 0] + 2.5) <= 0.05
    again = A.register(X1, case["C"], None, 1, kind="z", init=reg)       # starting from the answer: one step
    assert again.n_iter == 1 and np.allclose(again.t, reg.t, atol=2e-3)


# ---------------------------------------------------------------- plugin
def stub_fit(X, C0, max_iter, tol_abs):
    f = R.lloyd_fit(np.asarray(X, dtype=np.float32), C0, max_iter=max_iter, tol=tol_abs)
    return f["labels"], f["centers"], f["inertia"], f["n_iter"]


def stub_assign(X, C):
    labels = R.assign(X, C)
    sq = R.sqdist_rows(X, C[labels])
    return labels, sq, float(sq.astype(np.float64).sum())


def same_layers(a, b):
    assert len(a) == len(b)
    for (da, pa, ka), (db, pb, kb) in zip(a, b):
        assert ka == kb and pa["name"] == pb["name"] and np.array_equal(da, db, equal_nan=True)
        assert set(pa) == set(pb)
        for key, va in pa.get("properties", {}).items():
            assert np.array_equal(va, pb["properties"][key], equal_nan=True), key


def test_plugin_without_register_is_unchanged():
    from pcm_amd import plugin
    clouds = A.two_days(1500)

    def forbidden(*a):
        raise AssertionError("register=None must not register")

    l0, r0 = plugin.kmeans_fuse(clouds, n_clusters=16, max_iter=8, fit=stub_fit)
    l1, r1 = plugin.kmeans_fuse(clouds, n_clusters=16, max_iter=8, fit=stub_fit, register=None, register_to=1,
                                register_max_dist=2.0, align=forbidden)
    same_layers(l0, l1)
    assert set(r0) == set(r1) and "registration" not in r1
    for key in r0:
        assert np.array_equal(r0[key], r1[key]), key
    a0, s0 = plugin.kmeans_assign(clouds[1:], r0, assign=stub_assign)
    a1, s1 = plugin.kmeans_assign(clouds[1:], r0, assign=stub_assign, register=None, align=forbidden)
    same_layers(a0, a1)
    assert set(s0) == set(s1)


def test_plugin_fuse_with_registration():
    from pcm_amd import plugin
    clouds = A.two_days(1500)
    layers, res = plugin.kmeans_fuse(clouds, n_clusters=16, max_iter=8, fit=stub_fit, register="rigid", align=A.ref_align)
    reg = res["registration"]
    assert reg["R"].shape == (2, 3, 3) and reg["t"].shape == (2, 3) and reg["transforms"].shape == (2, 12)
    assert np.array_equal(reg["R"][0], np.eye(3)) and not reg["t"][0].any()           # the reference cloud stays
    assert reg["n_iter"] >= 1 and reg["inliers"].tolist() == [0, 1500] and reg["rms_after"][1] <= reg["rms_before"][1]
    # the model the others were registered to is that of cloud 0 alone
    _, base = plugin.kmeans_fuse(clouds[:1], n_clusters=16, max_iter=8, fit=stub_fit)
    X1 = clouds[1].astype(np.float32)
    want = A.register(X1, base["centers"], np.zeros(1500, np.uint8), 1, kind="rigid")
    assert np.array_equal(reg["transforms"][1], want.transforms[0])
    moved = A.transform(X1, want.transforms)
    fused = layers[1][0]
    assert np.array_equal(fused[:1500], clouds[0].astype(np.float32).astype(np.float64))
    assert np.array_equal(fused[1500:], moved.astype(np.float64)) and not np.array_equal(moved, X1)
    # the fuse itself is the existing one, on the registered points
    l2, r2 = plugin.kmeans_fuse([clouds[0], moved.astype(np.float64)], n_clusters=16, max_iter=8, fit=stub_fit)
    same_layers(layers, l2)
    assert np.array_equal(res["labels"], r2["labels"]) and np.array_equal(res["centers"], r2["centers"])
    # register_to picks the other cloud
    _, res1 = plugin.kmeans_fuse(clouds, n_clusters=16, max_iter=8, fit=stub_fit, register="z", register_to=1,
                                 align=A.ref_align)
    assert not res1["registration"]["t"][1].any() and res1["registration"]["t"][0, 0] != 0
    assert not res1["registration"]["t"][0, 1:].any()


def test_plugin_assign_with_registration_measures_change_not_offset():
    from pcm_amd import plugin
    clouds = A.two_days(1500)
    _, model = plugin.kmeans_fuse(clouds[:1], n_clusters=16, max_iter=8, fit=stub_fit)
    _, plain = plugin.kmeans_assign(clouds[1:], model, assign=stub_assign)
    layers, res = plugin.kmeans_assign(clouds[1:], model, assign=stub_assign, register="rigid", align=A.ref_align)
    assert res["registration"]["R"].shape == (1, 3, 3) and res["registration"]["inliers"].tolist() == [1500]
    assert res["inertia"] < plain["inertia"]
    assert not np.array_equal(layers[0][0], clouds[1].astype(np.float32).astype(np.float64))


def test_plugin_errors_come_back_as_error_layers():
    from pcm_amd import plugin
    clouds = A.two_days(300)

    class Base:
        def run(self, kml_path, **kw):
            return [(c, {"name": f"pair {i} {plugin.CLOUD_LAYER_SUFFIX}"}, "points") for i, c in enumerate(clouds)]

    def broken(*a):
        raise RuntimeError("registration failed")

    for kw, word in ((dict(register="affine", align=A.ref_align), "register must be"),
                     (dict(register="rigid", register_to=5, align=A.ref_align), "register_to"),
                     (dict(register="rigid", align=broken), "registration failed")):
        out = plugin.HeightMapExtractor(base=Base(), n_clusters=8, max_iter=4, fit=stub_fit, **kw).run("x.kml")
        assert len(out) == 1 and out[0][1]["name"].startswith("Error:") and word in out[0][1]["name"], (kw, out[0][1])
    ex = plugin.HeightMapExtractor(base=Base(), n_clusters=8, max_iter=4, fit=stub_fit, register="translation",
                                   align=A.ref_align)
    out = ex.run("x.kml")
    assert len(out) == 4 and ex.last_result["registration"]["t"].shape == (2, 3)
    with pytest.raises(ValueError):
        plugin.kmeans_fuse(clouds, n_clusters=8, fit=stub_fit, register="rigid", register_to=-1, align=A.ref_align)
