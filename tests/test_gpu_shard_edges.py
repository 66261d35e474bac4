"""The slab sharding operators on the GPU against tests/shard_ref.py, directly:
``engine.shard_hist`` (k_shard_hist), ``engine.shard_partition`` (k_shard_count,
the scan, k_shard_totals, k_shard_scatter) and ``engine.shard_scatter_labels``
(k_shard_labels).  A whole fit does not notice a row in the wrong bin, a
partition in the wrong order or a histogram that disagrees with the partition;
these tests do.  The inputs are tests/shard_cases.py's (the same ones
tests/test_shard_ref.py gives the CPU restatement): sizes on the ballot, round
and block edges of the scatter, the destination patterns a rank-by-ballot
scatter can get wrong, up to 16 ranks, both dtypes, every d and axis, values on
and next to bin edges, and global rows up to 2^32 - 2.

All outputs are integers or bit patterns: every comparison is exact.
"""
import ctypes

import numpy as np
import pytest

import shard_cases as SC
import shard_ref as S


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pcm_amd import engine, lloyd
    return torch, engine, lloyd


def check(gpu, c):
    """Every promise of the three operators on one case."""
    torch, E, lloyd = gpu
    X = torch.from_numpy(c.X).cuda()
    words = np.int32 if c.dtype == "f32" else np.int16

    h = E.shard_hist(X, c.axis, c.lo, c.inv, c.nbins)
    assert h.dtype == torch.int64 and tuple(h.shape) == (c.nbins,)
    h = h.cpu().numpy()
    np.testing.assert_array_equal(h, S.hist(c.X, c.axis, c.lo, c.inv, c.nbins))
    assert int(h.sum()) == c.n

    order, rows_ref, counts_ref = S.partition(c.X, c.axis, c.lo, c.inv, c.nbins, c.owner, c.P, c.gidx0)
    Xo, rows, counts = E.shard_partition(X, c.axis, c.lo, c.inv, c.nbins, c.owner, c.P, c.gidx0)
    assert counts.dtype == np.int64 and rows.dtype == torch.int32 and Xo.dtype == X.dtype
    assert tuple(Xo.shape) == (c.n, c.d) and tuple(rows.shape) == (c.n,)
    np.testing.assert_array_equal(counts, counts_ref)
    np.testing.assert_array_equal(rows.cpu().numpy().view(np.uint32), rows_ref)              # stable: the one order
    np.testing.assert_array_equal(Xo.cpu().numpy().view(words), c.X[order].view(words))      # a bit-for-bit payload
    np.testing.assert_array_equal(lloyd.slab_sizes(h, c.owner, c.P), counts)                # the capacity gate's numbers

    labels = np.random.default_rng(c.n).integers(-1, 1 << 20, c.n).astype(np.int32)
    back = E.shard_scatter_labels(torch.from_numpy(labels[order]).cuda(), rows, c.gidx0, c.n)
    assert back.dtype == torch.int32 and tuple(back.shape) == (c.n,)
    np.testing.assert_array_equal(back.cpu().numpy(), labels)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SC.part_names())
def test_partition_patterns(gpu, name):
    check(gpu, SC.build(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SC.bins_names())
def test_bin_edges(gpu, name):
    check(gpu, SC.build(name))


@pytest.mark.gpu
@pytest.mark.parametrize("gidx", SC.GIDX)
@pytest.mark.parametrize("n", [n for n in SC.SIZES if n])
def test_round_trip_at_every_size_and_offset(gpu, n, gidx):
    """Rows and the label round trip at every scatter edge with every kind of gidx0, 16 ranks."""
    c = SC.build(f"part-uniform-n{n}")
    rng = np.random.default_rng(n)
    c.P, c.gidx, c.gidx0 = SC.MAXP, gidx, SC.gidx0_of(gidx, n)
    c.owner = SC.permuted_owner(c.nbins, c.P, rng)
    assert c.gidx0 + n <= 2 ** 32 - 1
    check(gpu, c)


@pytest.mark.gpu
def test_histogram_grid_stride(gpu):
    """More than two trips of k_shard_hist's grid-stride loop (its grid is capped at two blocks per CU)."""
    torch = gpu[0]
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    c = SC.build_stride(ncu)
    assert c.n > 2 * (2 * ncu * SC.TPB) and c.X.nbytes < 4 << 20
    check(gpu, c)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", list(SC.DTYPES))
def test_empty_shard(gpu, dtype):
    """n = 0: empty outputs, zero counts, a zeroed histogram, and no launch error left behind."""
    torch, E, _ = gpu
    for d in (1, 2, 3, 4):
        X = torch.empty((0, d), dtype=getattr(torch, {"f32": "float32", "f16": "float16"}[dtype]), device="cuda")
        for P, gidx0 in ((1, 0), (16, 12345), (3, 2 ** 32 - 1)):
            h = E.shard_hist(X, d - 1, 0.5, 3.0, 1000)
            assert h.dtype == torch.int64 and h.cpu().numpy().tolist() == [0] * 1000
            Xo, rows, counts = E.shard_partition(X, d - 1, 0.5, 3.0, 1000, np.zeros(1000, np.uint8), P, gidx0)
            assert tuple(Xo.shape) == (0, d) and tuple(rows.shape) == (0,) and counts.tolist() == [0] * P
            back = E.shard_scatter_labels(torch.empty(0, dtype=torch.int32, device="cuda"), rows, gidx0, 0)
            assert tuple(back.shape) == (0,) and back.dtype == torch.int32
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_workspace_one_byte_short(gpu):
    """The partition refuses a workspace smaller than its own size query, before any launch."""
    torch, E, _ = gpu
    from pcm_amd import _lib
    lib = _lib.load()
    c = SC.build("part-uniform-n4097")
    X = torch.from_numpy(c.X).cuda()
    own = torch.from_numpy(c.owner).cuda()
    out, rows = torch.empty_like(X), torch.full((c.n,), -7, dtype=torch.int32, device="cuda")
    counts = np.full(c.P, -1, np.int64)
    need = ctypes.c_size_t()
    assert lib.pcm_shard_partition_workspace(c.n, c.P, ctypes.byref(need)) == 0 and need.value > 0
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")

    def call(nbytes):
        return lib.pcm_shard_partition(E._ptr(X), E._dtype_code(X), c.n, c.d, c.axis, c.lo, c.inv, c.nbins, E._ptr(own),
                                       c.P, c.gidx0, E._ptr(out), E._ptr(rows), counts.ctypes.data_as(ctypes.c_void_p),
                                       E._ptr(ws), nbytes, E._stream())

    assert call(need.value - 1) == -1
    assert "pcm_shard_partition: workspace too small" in _lib.last_error()
    torch.cuda.synchronize()
    assert (rows.cpu().numpy() == -7).all()                                  # nothing ran
    assert call(need.value) == 0                                             # and the queried size is enough
    order, rows_ref, counts_ref = S.partition(c.X, c.axis, c.lo, c.inv, c.nbins, c.owner, c.P, c.gidx0)
    np.testing.assert_array_equal(counts, counts_ref)
    np.testing.assert_array_equal(rows.cpu().numpy().view(np.uint32), rows_ref)
