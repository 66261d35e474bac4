"""CPU: the slab sharding contract without a device.

* tests/cpu_engine.py's restatement of csrc/pcm_shard.hip (what every gloo test
  of the multi-rank driver runs on) against tests/shard_ref.py, on the inputs
  tests/test_gpu_shard_edges.py gives the HIP operators;
* ``lloyd.slab_sizes`` against the reference's partition counts;
* the case list itself: every value the operators branch on is drawn, together
  with the others it has to meet;
* the entry points' argument rejections that return before any device call.
"""
import ctypes
import os

import numpy as np
import pytest

import shard_cases as SC
import shard_ref as S


# ---------------------------------------------------------------- the reference, row by row
def test_reference_against_a_python_loop():
    """shard_ref's vector code against the contract's words applied to one row at a time."""
    import math
    c = SC.build("bins-affine-b1000-f32")
    order_of = [[] for _ in range(c.P)]
    h = [0] * c.nbins
    for i in range(c.n):
        t = math.floor((float(c.X[i, c.axis]) - c.lo) * c.inv)
        b = min(max(t, 0), c.nbins - 1)
        h[b] += 1
        order_of[int(c.owner[b])].append(i)
    order, rows, counts = S.partition(c.X, c.axis, c.lo, c.inv, c.nbins, c.owner, c.P, c.gidx0)
    assert S.hist(c.X, c.axis, c.lo, c.inv, c.nbins).tolist() == h
    assert order.tolist() == sum(order_of, [])
    assert counts.tolist() == [len(o) for o in order_of]
    assert rows.tolist() == [(i + c.gidx0) % 2 ** 32 for i in sum(order_of, [])]


def test_reference_clamps_what_no_integer_holds():
    X = np.asarray([[3e38], [-3e38], [0.5]], np.float32)
    assert S.bins(X, 0, 0.0, 16384.0, 16384).tolist() == [16383, 0, 8192]
    assert S.bins(X, 0, -3e38, 1e300, 7).tolist() == [6, 0, 6]


# ---------------------------------------------------------------- the case list
def test_cases_cover_what_the_operators_branch_on():
    cases = [SC.build(name) for name in SC.names()]
    part = [c for c in cases if c.name.startswith("part-")]
    assert {(c.name.split("-")[1], c.n) for c in part} >= {(p, n) for p in SC.PATTERNS for n in SC.SIZES}
    assert {(c.P, c.dtype) for c in part} >= {(P, t) for P in SC.RANKS for t in SC.DTYPES}
    assert {(c.d, c.axis, c.dtype) for c in part} >= {(d, a, t) for d in (1, 2, 3, 4) for a in range(d) for t in SC.DTYPES}
    assert {c.nbins for c in part} >= {16, 512, 1000, 1024, 16384}
    big = [c for c in part if c.n > SC.CHUNK]                      # more than one scatter block
    assert {c.P for c in big} >= set(SC.RANKS) and {c.d for c in big} == {1, 2, 3, 4}
    assert {(c.gidx, c.dtype) for c in big} >= {(g, t) for g in SC.GIDX for t in SC.DTYPES}
    top = [c for c in big if c.gidx == "top"]
    assert top and all(c.gidx0 + c.n == 2 ** 32 - 1 and c.gidx0 + c.n // 2 > 2 ** 31 for c in top)
    edge = [c for c in cases if c.name.startswith("bins-")]
    assert {(c.name.split("-")[1], c.nbins, c.dtype) for c in edge} == \
        {(k, b, t) for k in SC.BIN_KINDS for b in SC.NBINS for t in SC.DTYPES}
    assert {c.P for c in edge} == set(SC.RANKS) and {c.d for c in edge} == {1, 2, 3, 4}
    for c in part:                                                 # the patterns are what their names say
        dest = S.dests(c.X, c.axis, c.lo, c.inv, c.nbins, c.owner)
        pattern = c.name.split("-")[1]
        if pattern == "midempty" and c.n > 256:
            assert c.P == 8 and set(dest.tolist()) == {0, 1, 6, 7}
        if pattern == "tail" and c.n > 1:
            assert (dest[:-1] == 0).all() and dest[-1] == c.P - 1 > 0
        if pattern == "permuted" and c.P > 2:
            assert (np.diff(c.owner.astype(int)) < 0).any()        # not monotone
        if pattern == "edges" and c.P > 1 and c.n > 4097:
            assert np.flatnonzero(np.diff(dest)).tolist() == [r - 1 for r in SC.RUNS]
    whole = SC.build(f"part-runs-n{sum(SC.RUNS) + 77}")
    dest = S.dests(whole.X, whole.axis, whole.lo, whole.inv, whole.nbins, whole.owner)
    if whole.P > 1:
        assert np.diff(np.flatnonzero(np.diff(dest)), prepend=-1).tolist()[:len(SC.RUNS)] == list(SC.RUNS)


def test_bin_cases_reach_the_edges_they_are_named_for():
    for nbins in SC.NBINS:
        c = SC.build(f"bins-grid-b{nbins}-f32")
        assert S.hist(c.X, c.axis, c.lo, c.inv, c.nbins).min() > 0            # every bin, from both of its ends
        c = SC.build(f"bins-hi-b{nbins}-f32")
        x = c.X[:, c.axis].astype(np.float64)
        assert ((x - c.lo) * c.inv >= nbins).any() and ((x - c.lo) * c.inv < 0).any()      # clamped at both ends
        c = SC.build(f"bins-flat-b{nbins}-f16")
        assert c.inv == 0.0 and S.hist(c.X, c.axis, c.lo, c.inv, c.nbins)[0] == c.n
        for t, tiny in (("f32", 2.0 ** -126), ("f16", 2.0 ** -14)):
            c = SC.build(f"bins-tiny-b{nbins}-{t}")
            x = c.X[:, c.axis]
            sub = (x != 0) & (np.abs(x.astype(np.float64)) < tiny)
            assert sub.sum() > 100 and np.signbit(x[x == 0]).any()
            assert len(np.unique(S.bins(c.X[sub], c.axis, c.lo, c.inv, c.nbins))) >= min(nbins, 1000)
        c = SC.build(f"bins-huge-b{nbins}-f32")
        t = (c.X[:, c.axis].astype(np.float64) - c.lo) * c.inv
        assert c.inv == 16384.0 and t.max() > 2.0 ** 64 and (t.min() < -2.0 ** 64 or c.lo < 0)
        assert abs(float(c.X[:, c.axis].max())) == np.float32(3e38)


# ---------------------------------------------------------------- tests/cpu_engine.py restates the same contract
def _oracle_engine(d):
    torch = pytest.importorskip("torch")
    from cpu_engine import OracleEngine
    return torch, OracleEngine(d, 2)


def check_restatement(c):
    torch, eng = _oracle_engine(c.d)
    from pcm_amd import lloyd
    X = torch.from_numpy(c.X)
    words = np.int32 if c.dtype == "f32" else np.int16
    h = eng.shard_hist(X, c.axis, c.lo, c.inv, c.nbins)
    assert h.dtype == torch.int64
    np.testing.assert_array_equal(h.numpy(), S.hist(c.X, c.axis, c.lo, c.inv, c.nbins))
    order, rows_ref, counts_ref = S.partition(c.X, c.axis, c.lo, c.inv, c.nbins, c.owner, c.P, c.gidx0)
    Xo, rows, counts = eng.shard_partition(X, c.axis, c.lo, c.inv, c.nbins, c.owner, c.P, c.gidx0)
    np.testing.assert_array_equal(counts, counts_ref)
    assert rows.dtype == torch.int32 and Xo.dtype == X.dtype
    np.testing.assert_array_equal(rows.numpy().view(np.uint32), rows_ref)
    np.testing.assert_array_equal(Xo.numpy().view(words), c.X[order].view(words))
    np.testing.assert_array_equal(lloyd.slab_sizes(h.numpy(), c.owner, c.P), counts_ref)
    labels = np.random.default_rng(c.n).integers(-1, 1 << 20, c.n).astype(np.int32)
    back = eng.shard_scatter_labels(torch.from_numpy(labels[order]), rows, c.gidx0, c.n)
    assert back.dtype == torch.int32
    np.testing.assert_array_equal(back.numpy(), labels)
    np.testing.assert_array_equal(S.scatter_labels(labels[order], rows_ref, c.gidx0, c.n), labels)


@pytest.mark.parametrize("name", SC.names())
def test_cpu_engine_restates_the_contract(name):
    check_restatement(SC.build(name))


def test_cpu_engine_on_the_grid_stride_cloud():
    check_restatement(SC.build_stride(256))


def test_rows_wrap_past_2_31():
    """gidx0 + n = 2^32 - 1: the int32 words are negative, the uint32 view is the global index."""
    c = SC.build("part-uniform-n4097")
    torch, eng = _oracle_engine(c.d)
    g0 = SC.gidx0_of("top", c.n)
    _, rows, _ = eng.shard_partition(torch.from_numpy(c.X), c.axis, c.lo, c.inv, c.nbins, c.owner, c.P, g0)
    order, rows_ref, _ = S.partition(c.X, c.axis, c.lo, c.inv, c.nbins, c.owner, c.P, g0)
    assert (rows.numpy() < 0).all() and rows_ref.max() == 2 ** 32 - 2
    np.testing.assert_array_equal(rows.numpy().view(np.uint32).astype(np.int64), order + g0)


# ---------------------------------------------------------------- slab_sizes and slab_owner
@pytest.mark.parametrize("name", [n for n in SC.names() if n.startswith("bins-")] + [f"part-uniform-n{n}" for n in SC.SIZES])
def test_slab_sizes_of_slab_owner_tables(name):
    """The capacity gate's numbers (histogram + owner table) are the partition's counts, for the
    tables the driver builds (lloyd.slab_owner) at every world size the partition addresses."""
    from pcm_amd import lloyd
    c = SC.build(name)
    h = S.hist(c.X, c.axis, c.lo, c.inv, c.nbins)
    for P in SC.RANKS:
        owner = lloyd.slab_owner(h, P)
        assert owner.dtype == np.uint8 and owner.shape == (c.nbins,) and (np.diff(owner.astype(int)) >= 0).all()
        assert c.n == 0 or owner.max() < P
        counts = S.partition(c.X, c.axis, c.lo, c.inv, c.nbins, owner, P, 0)[2]
        sizes = lloyd.slab_sizes(h, owner, P)
        assert sizes.dtype == np.int64 and sizes.shape == (P,)
        np.testing.assert_array_equal(sizes, counts)


# ---------------------------------------------------------------- rejections before any device call
@pytest.fixture(scope="module")
def lib():
    from pcm_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.load(require_gpu_runtime=False)


def _host(nbytes=64):
    """A host buffer standing in for a pointer a rejected call never follows."""
    buf = ctypes.create_string_buffer(nbytes)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_shard_argument_errors_without_device(lib):
    """Each case fails in the entry point's argument checks, before any device call:
    -1 (PCM_E_ARG) and a message that names the entry point."""
    from pcm_amd import _lib
    from pcm_amd.engine import PCM_F16, PCM_F32
    keep, p = _host()

    def rejected(rc, entry):
        assert rc == -1
        assert _lib.last_error().startswith(entry + ":"), _lib.last_error()

    def hist(dtype=PCM_F32, n=4, d=3, axis=0, nbins=16):
        return lib.pcm_shard_hist(p, dtype, n, d, axis, 0.0, 1.0, nbins, p, None)

    rejected(hist(nbins=0), "pcm_shard_hist")
    rejected(hist(nbins=SC.HIST_BINS_MAX + 1), "pcm_shard_hist")
    rejected(hist(d=3, axis=3), "pcm_shard_hist")
    rejected(hist(d=5), "pcm_shard_hist")
    for code in (2, -1, 7):                                       # PCM_F64 is the dense path's only
        rejected(hist(dtype=code), "pcm_shard_hist")
        rejected(hist(dtype=code, n=0), "pcm_shard_hist")
        assert "dtype" in _lib.last_error()
    assert PCM_F16 == 1 and PCM_F32 == 0

    nbytes = ctypes.c_size_t(77)
    for P in (0, SC.MAXP + 1):
        rejected(lib.pcm_shard_partition_workspace(4096, P, ctypes.byref(nbytes)), "pcm_shard_partition_workspace")
    assert nbytes.value == 77

    def partition(n, gidx0):
        return lib.pcm_shard_partition(p, PCM_F32, n, 3, 0, 0.0, 1.0, 16, p, 2, gidx0, p, p, p, p, 1 << 20, None)

    rejected(partition(5, -1), "pcm_shard_partition")
    rejected(partition(5, 2 ** 32 - 5), "pcm_shard_partition")     # gidx0 + n = 2^32: the last row has no uint32 word
    rejected(partition(0, 2 ** 32), "pcm_shard_partition")
    del keep
