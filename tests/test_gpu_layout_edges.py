"""The layout ``pcm_layout_build`` leaves on the GPU against tests/layout_ref.py, directly: the
bounding box, the grid, the sort plan, ``perm`` and ``xs`` (the stable (key, row) order of the LSD
record sort), the cell and sub-cell starts, the tile table, the per-tile fixed-point sums, the
compressed stream, the tile boxes of crowded layouts, the position maps, and the four ways
``pcm_labels`` carries labels back to the caller's row order.  A whole fit notices a point in the
wrong cell; it does not notice a wrong order inside a sub-cell, a record written beside its
field, a tile sum nobody happens to use or a scan that only breaks past 256 chunks.  The inputs
are tests/layout_cases.py's; tests/test_layout_ref.py asserts on the CPU that each reaches the
edge it is named for.

Everything the layout holds is an integer or a bit pattern: every comparison is exact.  Two
boxes are compared by value, since the sign of a zero extreme is not defined: the bounding box and
the tile boxes.
"""
import ctypes
import time

import numpy as np
import pytest

import layout_cases as LC
import layout_ref as LR

pytestmark = pytest.mark.gpu

FACTS = ("sub", "zlev", "tile_cap", "npad", "ntiles", "ntiles_cap", "bits", "npass", "wb", "nblk", "nseg", "has_dmap",
         "use_xz", "tiles_lpt", "label_bytes", "ncells", "n", "d", "prune", "k")
KNOBS = ("PCM_CELL_TARGET", "PCM_TILE_CAP", "PCM_ZLEV", "PCM_TILE_LPT")
PCM_E_STATE, PCM_E_NONFINITE = -3, -4


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pcm_amd import _lib, engine, lloyd
    lib = _lib.load()
    P = ctypes.c_void_p
    lib.pcm_debug_layout.argtypes, lib.pcm_debug_layout.restype = [P] * 5, ctypes.c_int
    lib.pcm_debug_layout_facts.argtypes, lib.pcm_debug_layout_facts.restype = [P, P, ctypes.c_int], ctypes.c_int
    lib.pcm_debug_layout_buffer.argtypes = [P, ctypes.c_char_p, P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), P]
    lib.pcm_debug_layout_buffer.restype = ctypes.c_int
    return torch, engine, lloyd, lib


def set_knobs(monkeypatch, env):
    for kn in KNOBS:
        if kn in env:
            monkeypatch.setenv(kn, env[kn])
        else:
            monkeypatch.delenv(kn, raising=False)


def facts(gpu, eng):
    out = np.zeros(len(FACTS), np.int64)
    assert gpu[3].pcm_debug_layout_facts(eng.h, out.ctypes.data, len(out)) == 0
    return dict(zip(FACTS, out.tolist()))


def buffer(gpu, eng, name, dtype, missing=False):
    """One named buffer of the layout as a numpy array (None when `missing` and the layout has none)."""
    torch, E, _, lib = gpu
    need = ctypes.c_size_t()
    rc = lib.pcm_debug_layout_buffer(eng.h, name.encode(), None, 0, ctypes.byref(need), None)
    if missing and rc == PCM_E_STATE:
        return None
    assert rc == 0, name
    out = torch.zeros(need.value + 8, dtype=torch.uint8, device="cuda")
    assert lib.pcm_debug_layout_buffer(eng.h, name.encode(), E._ptr(out), need.value + 8, None, E._stream()) == -1
    assert lib.pcm_debug_layout_buffer(eng.h, name.encode(), E._ptr(out), need.value, None, E._stream()) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()[: need.value].view(dtype)


def sorted_cloud(gpu, eng, f, np_dtype):
    """(xs, perm, sorted-order labels) through pcm_debug_layout."""
    torch, E, _, lib = gpu
    xs = torch.empty(f["d"] * f["npad"], dtype=torch.float16 if np_dtype == np.float16 else torch.float32, device="cuda")
    lab = torch.empty(f["n"], dtype=torch.int32, device="cuda")
    perm = torch.empty(f["n"], dtype=torch.int32, device="cuda")
    assert lib.pcm_debug_layout(eng.h, E._ptr(xs), E._ptr(lab), E._ptr(perm), E._stream()) == 0
    torch.cuda.synchronize()
    return xs.cpu().numpy(), perm.cpu().numpy().view(np.uint32).astype(np.int64), lab.cpu().numpy()


def check(gpu, monkeypatch, c, Xt=None, timed=None):
    """Every promise of the layout on one case.  Xt: the cloud already on the device (an unaligned view)."""
    torch, E, lloyd, lib = gpu
    set_knobs(monkeypatch, c.env)
    words = np.int32 if c.dtype == "f32" else np.int16
    if Xt is None:
        Xt = torch.from_numpy(c.X).cuda()
    eng = E.Engine(c.d, c.k, Xt.dtype)
    p = LR.plan(c.X, c.k, c.env)
    L = LR.build(p, c.X)

    lo, hi, mx = eng.bbox(Xt)
    np.testing.assert_array_equal(lo, p.lo)                 # by value
    np.testing.assert_array_equal(hi, p.hi)
    np.testing.assert_array_equal(mx, np.maximum(np.abs(p.lo), np.abs(p.hi)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    q, _ = lloyd.prepare(eng, Xt, lloyd.LOCAL)
    if timed is not None:
        timed.append(time.perf_counter() - t0)
    assert list(q) == p.q.tolist()

    f = facts(gpu, eng)
    want = dict(sub=p.sub, zlev=p.zlev, tile_cap=p.tile_cap, npad=p.npad, ntiles=L.ntiles, ntiles_cap=p.ntiles_cap,
                bits=p.bits, npass=p.npass, wb=p.wb, nblk=p.nblk, nseg=p.nseg, has_dmap=p.has_dmap, use_xz=p.use_xz,
                tiles_lpt=0, label_bytes=p.label_bytes, ncells=p.ncells, n=c.n, d=c.d, prune=p.g.prune, k=c.k)
    assert f == want
    info = eng.layout_info()
    assert info == dict(ncells=p.ncells, ntiles=L.ntiles, grid=p.g.G)

    xs, perm, _ = sorted_cloud(gpu, eng, f, c.X.dtype)
    np.testing.assert_array_equal(perm, L.perm)             # the stable (key, row) order, the one order
    np.testing.assert_array_equal(xs.view(words), L.xs.view(words))            # bit for bit, the zero padding included
    if p.zlev == 0:
        np.testing.assert_array_equal(buffer(gpu, eng, "sub_start", np.uint32), L.sub_start)
    else:
        assert buffer(gpu, eng, "sub_start", np.uint32, missing=True) is None
    np.testing.assert_array_equal(buffer(gpu, eng, "cell_start", np.uint32), L.cell_start)
    np.testing.assert_array_equal(buffer(gpu, eng, "tile_off", np.uint32), L.tile_off)
    tiles = buffer(gpu, eng, "tiles", np.uint32).reshape(-1, 4)
    np.testing.assert_array_equal(tiles, L.tiles)
    np.testing.assert_array_equal(buffer(gpu, eng, "tsum", np.int64).reshape(-1, c.d), L.tsum)

    dmap = buffer(gpu, eng, "dmap", np.uint32, missing=True)
    assert (dmap is not None) == bool(p.has_dmap)
    if dmap is not None:                                    # row -> position after pass 1 -> sorted position
        d0, d1 = dmap[: c.n].astype(np.int64), dmap[c.n:].astype(np.int64)
        for m in (d0, d1):
            np.testing.assert_array_equal(np.sort(m), np.arange(c.n))
        np.testing.assert_array_equal(L.perm[d1[d0]], np.arange(c.n))

    tmeta = buffer(gpu, eng, "tmeta", np.uint32, missing=True)
    assert (tmeta is not None) == bool(p.use_xz)
    zpts = int(buffer(gpu, eng, "zpts", np.uint64).reshape(32, 16)[:, 0].sum())
    sb = eng.stream_bytes()
    assert zpts == sb["compressed_points"] == L.compressed_points
    assert sb["bytes"] == L.stream_bytes
    if tmeta is not None:
        tmeta = tmeta.reshape(-1, 4)
        np.testing.assert_array_equal(tmeta, L.tmeta)
        xz = buffer(gpu, eng, "xz", np.uint32)
        pos, pat = LR.decode(tmeta, xz, tiles.astype(np.int64))
        U = np.ascontiguousarray(c.X[L.perm]).view(np.uint32)
        np.testing.assert_array_equal(pat, U[pos])          # lossless: the stream rebuilds xs bit for bit
        if len(pos):                                        # and the records themselves, word for word
            got = xz[LR.zword(pos)].astype(np.uint64) | (xz[LR.zword(pos) + LR.ZHI].astype(np.uint64) << np.uint64(32))
            np.testing.assert_array_equal(got, L.rec[pos])

    tbox = buffer(gpu, eng, "tbox", np.float32, missing=True)
    assert (tbox is not None) == (p.zlev > 0)
    if tbox is not None:
        np.testing.assert_array_equal(tbox.reshape(-1, 2, 4), L.tbox)          # by value
    assert buffer(gpu, eng, "torig", np.uint32, missing=True) is None
    assert lib.pcm_debug_layout_buffer(eng.h, b"nonesuch", None, 0, None, None) == -1
    eng.close()
    return p, L


@pytest.mark.parametrize("name", LC.edge_names())
def test_chunk_and_wave_edges(gpu, monkeypatch, name):
    check(gpu, monkeypatch, LC.build(name))


@pytest.mark.parametrize("name", LC.vec_names())
@pytest.mark.parametrize("aligned", [True, False])
def test_vec_rows_and_unaligned_cloud(gpu, monkeypatch, name, aligned):
    """The 16-byte row loads of the first count pass and their tail; the same cloud 12 bytes off
    alignment (`big[1:]`, contiguous) takes the 4-byte loads and must give the identical layout."""
    torch = gpu[0]
    c = LC.build(name)
    big = torch.zeros((c.n + 1, 3), dtype=torch.float32, device="cuda")
    big[1:] = torch.from_numpy(c.X).cuda()
    Xt = big[1:].clone() if aligned else big[1:]
    assert Xt.is_contiguous() and Xt.data_ptr() % 16 == (0 if aligned else 12)
    check(gpu, monkeypatch, c, Xt)


@pytest.mark.parametrize("name", LC.pass_names())
def test_pass_counts(gpu, monkeypatch, name):
    check(gpu, monkeypatch, LC.build(name))


@pytest.mark.parametrize("name", LC.SEG_NAMES)
def test_segment_scan(gpu, monkeypatch, name):
    """One segment of 256 chunks, two, and the nine that enter k_rs_segscan's unrolled loop; the box's
    extremes in the last rows (k_bbox_partial's 4-row loop and its tail)."""
    timed = []
    check(gpu, monkeypatch, LC.build(name), timed=timed)
    print(f"{name}: bbox + layout {timed[0] * 1e3:.1f} ms on the GPU")


@pytest.mark.parametrize("name", LC.SKEW_NAMES + LC.TILE_NAMES + LC.XZ_NAMES + LC.CROWD_NAMES)
def test_skew_tiles_compression_crowded(gpu, monkeypatch, name):
    check(gpu, monkeypatch, LC.build(name))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("where", ["first", "last", "unrolled", "tail"])
@pytest.mark.parametrize("bad", ["nan", "inf", "-inf"])
def test_bbox_refuses_non_finite(gpu, dtype, where, bad):
    """NaN or an infinity in the first row, the last row, a row the 4-row unrolled loop reads as its third
    (the first and the last are its first and fourth), or a row left to the loop after it."""
    torch, E, _, lib = gpu
    n = 3 * 1024 * 256 + 1024 + 3
    X = torch.rand((n, 3), device="cuda").to(torch.float16 if dtype == "f16" else torch.float32)
    row = {"first": 0, "last": n - 1, "unrolled": 2 * 1024 * 256 + 5, "tail": 1024 * 256 + 2000}[where]
    X[row, 1] = float(bad)
    eng = E.Engine(3, 8, X.dtype)
    out = [np.zeros(3) for _ in range(3)]
    rc = lib.pcm_layout_bbox(eng.h, E._ptr(X), n, E._stream(), *(o.ctypes.data_as(ctypes.c_void_p) for o in out))
    assert rc == PCM_E_NONFINITE
    X[row, 1] = 0.5
    assert lib.pcm_layout_bbox(eng.h, E._ptr(X), n, E._stream(), *(o.ctypes.data_as(ctypes.c_void_p) for o in out)) == 0
    eng.close()


# ------------------------------------------------------------------ labels back to the caller's row order
def _big_k_cloud(dmap):
    rng = np.random.default_rng(65536 + dmap)
    X = rng.uniform(0, 1, (70001, 3)).astype(np.float32)
    return LC._case("labels-k65536", X, 65536, {"PCM_CELL_TARGET": "64"} if dmap else {})


LABEL_CASES = {
    # name: (case, passes, label bytes): which way back pcm_labels takes follows from them and the output's alignment
    "dmap-n%4=0": (lambda: LC.build("vec-n16384"), 2, 2),
    "dmap-n%4=1": (lambda: LC.build("vec-n16385"), 2, 2),
    "dmap-n%4=3": (lambda: LC.build("vec-n16387"), 2, 2),
    "one-pass-tail": (lambda: LC.build("tiles-onecell"), 1, 2),
    "one-pass": (lambda: LC.build("pass-b8"), 1, 2),
    "three-pass": (lambda: LC.build("pass-b17"), 3, 2),
    "k65536-dmap": (lambda: _big_k_cloud(1), 2, 4),
    "k65536": (lambda: _big_k_cloud(0), 1, 4),
    "n=3": (lambda: LC.build("edge-f32d3-n3"), 2, 2),                          # the gathers' tail alone
    "n=1": (lambda: LC.build("edge-f32d3-n1"), 1, 2),
}


@pytest.mark.parametrize("name", list(LABEL_CASES))
def test_labels_return_to_row_order(gpu, monkeypatch, name):
    """After begin and final: labels()[perm[i]] == the sorted-order label i, whatever the assign kernel
    chose, into an aligned output and into one 4 bytes off (the gathers' and the scatter's other variants)."""
    torch, E, lloyd, lib = gpu
    make, npass, lbytes = LABEL_CASES[name]
    c = make()
    set_knobs(monkeypatch, c.env)
    Xt = torch.from_numpy(c.X).cuda()
    eng = E.Engine(c.d, c.k, Xt.dtype, max_iter=4)
    lloyd.prepare(eng, Xt, lloyd.LOCAL)
    f = facts(gpu, eng)
    assert (f["npass"], f["label_bytes"], f["has_dmap"]) == (npass, lbytes, int(npass == 2))
    rng = np.random.default_rng(c.n)
    rows = rng.choice(c.n, c.k, replace=c.k > c.n)
    eng.begin(torch.from_numpy(np.ascontiguousarray(c.X[rows])).cuda(), 0.0, 4)
    eng.final()
    _, perm, lab = sorted_cloud(gpu, eng, f, c.X.dtype)
    assert lab.min() >= 0 and lab.max() < c.k and (c.n < 100 or len(np.unique(lab)) > min(c.k, c.n) // 4)
    want = np.empty(c.n, np.int32)
    want[perm] = lab
    buf = torch.full((c.n + 8,), -7, dtype=torch.int32, device="cuda")
    for off in (0, 1, 2):
        out = buf[off: off + c.n]
        assert out.data_ptr() % 16 == 4 * off
        buf.fill_(-7)
        assert lib.pcm_labels(eng.h, E._ptr(out), E._stream()) == 0
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        np.testing.assert_array_equal(got[off: off + c.n], want)
        assert (got[:off] == -7).all() and (got[off + c.n:] == -7).all()       # nothing written beside the output
    np.testing.assert_array_equal(eng.labels().cpu().numpy(), want)
    eng.close()


# ------------------------------------------------------------------ tile reorder
@pytest.mark.parametrize("name", ["tiles-cap512", "xz-straddle", "edge-f16d3-n8193"])
def test_tile_reorder_moves_everything_with_its_tile(gpu, monkeypatch, name):
    """PCM_TILE_LPT=1, after begin: the table is a permutation of the layout's, tsum and tmeta moved with
    their tiles, tpos inverts torig, and the order is stable and non-increasing in the cell's list length."""
    torch, E, lloyd, lib = gpu
    c = LC.build(name)
    set_knobs(monkeypatch, {**c.env, "PCM_TILE_LPT": "1"})
    Xt = torch.from_numpy(c.X).cuda()
    eng = E.Engine(c.d, c.k, Xt.dtype, max_iter=4)
    lloyd.prepare(eng, Xt, lloyd.LOCAL)
    p = LR.plan(c.X, c.k, c.env)
    L = LR.build(p, c.X)
    rows = np.random.default_rng(1).choice(c.n, c.k, replace=False)
    eng.begin(torch.from_numpy(np.ascontiguousarray(c.X[rows]).astype(np.float32)).cuda(), 0.0, 4)
    f = facts(gpu, eng)
    assert f["tiles_lpt"] == 1 and f["ntiles"] == L.ntiles
    torig = buffer(gpu, eng, "torig", np.uint32).astype(np.int64)
    tpos = buffer(gpu, eng, "tpos", np.uint32).astype(np.int64)
    np.testing.assert_array_equal(np.sort(torig), np.arange(L.ntiles))
    np.testing.assert_array_equal(tpos[torig], np.arange(L.ntiles))
    # {cell, a, b}: the fourth word is the list builders' owner word by now (sole-owner tiles)
    np.testing.assert_array_equal(buffer(gpu, eng, "tiles", np.uint32).reshape(-1, 4)[:, :3], L.tiles[torig, :3])
    np.testing.assert_array_equal(buffer(gpu, eng, "tsum", np.int64).reshape(-1, c.d), L.tsum[torig])
    if p.use_xz:
        np.testing.assert_array_equal(buffer(gpu, eng, "tmeta", np.uint32).reshape(-1, 4), L.tmeta[torig])
    cnt = buffer(gpu, eng, "fc_cnt", np.uint32).astype(np.int64)[L.tiles[torig, 0]]
    length = np.where(cnt == 0xFFFFFFFF, 0xFFFF, np.minimum(cnt, 0xFFFE))     # FULL first
    assert (np.diff(length) <= 0).all()
    assert (np.diff(torig)[np.diff(length) == 0] > 0).all()                    # stable
    eng.close()
