"""GPU: the lean rounds of k_lloyd1 for short-list tiles.

A tile whose candidate list is no longer than the lane slots takes rounds that
carry no slot map and no overflow test, and whole rounds take their slot
addresses straight from the winner, with no in-tile test.  None of it may
change a result, so every fit here is compared bit for bit with
oracle.lloyd_ref (labels, centres, n_iter, shift history, the iterations at
which the statistics stopped changing, the exact inertia) and with the same
fit under PCM_FAST=0, which sends every tile through the generic rounds.

The clouds are built cell by cell (`_box`): a cube of G^3 cells with a chosen
number of points in each, so that the tile structure is known -- several tiles
per cell at PCM_TILE_CAP=512, starts that are no multiple of 4, ends that fall
mid-round, tiles below 512 points (no whole round) and one of exactly 4096 --
and is asserted through the layout's cell and tile counts.  The coordinate
ranges are those where a fixed-point sum could go wrong if the accumulation
ever took a short cut through the bit pattern (one exponent per axis, mixed
exponents, truncating small values, both signs, a constant axis, axes of very
different scale); the boxes are narrow enough for k_tile_compress to take
their tiles (three delta widths within 64 bits: a cell of a 6^3 grid over
[0.25, 1)^3 spans 3 x 22 bits and stays raw), and
`stream_bytes()["compressed_points"]` says which cases are compressed and which
partly raw.  The engine reports the mean and the longest list and the
sole-owner tiles, not a histogram: the cases assert those (a sole tile: length
1; a mean between 1 and 6; the clustered seeds' longest list past the 8 slots,
so the generic rounds run in the same launch as the lean ones).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import lloyd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pcm_amd
    return pcm_amd


def _box(lo, size, G, counts, seed):
    """Points of a cube [lo, lo + size)^3 cut into G^3 cells, counts[c] of them in the
    inner 80 % of cell c (row-major), plus the cube's two corners (they pin the
    engine's bounding box, so its grid is this one).  Rows are shuffled."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.size == G ** 3
    cell = np.repeat(np.arange(G ** 3), counts)
    idx = np.stack([cell // (G * G), (cell // G) % G, cell % G], axis=1).astype(np.float64)
    u = 0.1 + 0.8 * rng.random((cell.size, 3))
    X = lo + (idx + u) * (size / G)
    corners = np.array([[lo] * 3, [lo + size * (1 - 1e-4)] * 3])
    X = np.concatenate([X, corners]).astype(np.float32)
    X = X[rng.permutation(X.shape[0])]
    counts = counts.copy()
    counts[0] += 1
    counts[-1] += 1
    return X, counts


def _ragged(G, seed, lo=150, hi=1400):
    """Odd and even cell populations: tile starts of every residue mod 4, several tiles per cell at cap 512."""
    c = np.random.default_rng(seed).integers(lo, hi, G ** 3)
    c[0] -= 1                      # the corner points _box adds to the first and the last cell
    c[-1] -= 1
    c[(c % 512) == 0] += 1         # no cell ends on a round's edge
    c[0] -= 1 if (c[0] + 1) % 512 == 0 else 0
    c[-1] -= 1 if (c[-1] + 1) % 512 == 0 else 0
    return c


# name -> (builder, K, PCM_TILE_CAP or None, iterations, compressed points: "all" | "most" | "some",
#          PCM_CELL_TARGET of the clouds that are not built cell by cell)
def _c_quarter():        # every axis an exact shift (s = 0 and 1: [0.5, 1) and [0.25, 0.5) at q = 25)
    return _box(0.45, 0.1, 5, _ragged(5, 1), 11)


def _c_offset():         # [480, 560)^3 of [300, 900): exponents 2^8 and 2^9, cells straddling 512
    return _box(480.0, 80.0, 5, _ragged(5, 2), 12)


def _c_trunc():          # [0.2, 0.3)^3: truncating axes below 0.25, exact above, both inside the straddling cells
    return _box(0.2, 0.1, 5, _ragged(5, 3), 13)


def _c_unit():           # [0, 1)^3, 16^3 cells: rows below 0.25 and below 2^-6, tiles of ~45 points (no whole round)
    return _box(0.0, 1.0, 16, np.random.default_rng(4).integers(30, 60, 16 ** 3), 14)


def _c_signed():         # [-1, 1)^3, 15^3 cells: negative tiles, and the middle cells straddle 0 (raw)
    return _box(-1.0, 2.0, 15, np.random.default_rng(5).integers(40, 70, 15 ** 3), 15)


def _c_sizes():          # default tile cap: one cell of exactly 4096 points, one of 4097, tiles below 512
    counts = np.random.default_rng(6).integers(600, 2500, 64)
    counts[0] = 4096 - 1          # + the corner point
    counts[5], counts[21], counts[22], counts[40] = 4097, 300, 511, 513
    return _box(0.5, 0.125, 4, counts, 16)


def _c_flat():           # one axis constant: field width 0
    rng = np.random.default_rng(7)
    X = np.empty((60_000, 3), dtype=np.float32)
    X[:, :2] = (0.5 + 0.1 * rng.random((60_000, 2))).astype(np.float32)
    X[:, 2] = np.float32(0.7)
    return X, None


def _c_axes():           # axis 0 in [0.45, 0.55): exact; axes 1 and 2 near 0, four binades under the few rows
    rng = np.random.default_rng(8)   # that set their q: they truncate -- per-axis mixing inside one fold
    X = np.empty((60_000, 3), dtype=np.float32)
    X[:, 0] = (0.45 + 0.1 * rng.random(60_000)).astype(np.float32)
    X[:, 1:] = (2.0 ** -12 * (1.0 + 0.2 * rng.random((60_000, 2)))).astype(np.float32)
    X[:8, 1:] = (2.0 ** -8 * (0.9 + 0.1 * rng.random((8, 2)))).astype(np.float32)
    return X, None


CASES = {
    "quarter": (_c_quarter, 12, 512, 5, "all", None),
    "offset": (_c_offset, 12, 512, 5, "all", None),
    "trunc": (_c_trunc, 12, 512, 5, "all", None),
    "unit": (_c_unit, 64, None, 4, "some", None),
    "signed": (_c_signed, 64, None, 4, "some", None),
    "sizes": (_c_sizes, 8, None, 6, "all", None),
    "flat": (_c_flat, 8, 512, 4, "all", 100),
    "axes": (_c_axes, 8, 512, 4, "most", 256),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(X, cell counts or None, C0, oracle fit with history); built once, never modified."""
    build, k, _, iters, _, _ = CASES[name]
    X, counts = build()
    X.setflags(write=False)
    C0 = X[R.init_indices(X.shape[0], k)].copy()
    ref = R.lloyd_fit(X, C0, max_iter=iters, tol=0.0, fast=True, history=True)
    return X, counts, C0, ref


def _fit(pcm, X, C0, iters, dtype=torch.float32, check=None):
    from pcm_amd import lloyd
    from pcm_amd.engine import Engine
    eng = Engine(X.shape[1], C0.shape[0], dtype, max_iter=iters)
    Xt = torch.from_numpy(np.array(X)).to("cuda", dtype)
    Ct = torch.from_numpy(np.array(C0, dtype=np.float32)).cuda()
    if check is not None:            # the layout and the lists of C0, before the fit
        lloyd.prepare(eng, Xt, lloyd.LOCAL)
        eng.begin(Ct, 0.0, iters)
        check(eng)
    res = pcm.lloyd_fit(Xt, Ct, max_iter=iters, tol=0.0, engine=eng)
    torch.cuda.synchronize()
    out = dict(labels=res.labels.cpu().numpy(), centers=res.centers.cpu().numpy(), n_iter=res.n_iter,
               inertia=res.inertia, changed=np.asarray(res.stat_words_changed), shift=np.asarray(res.shift))
    eng.close()
    return out


def _assert_oracle(got, ref, where):
    assert got["n_iter"] == ref["n_iter"], f"{where}: n_iter {got['n_iter']} != {ref['n_iter']}"
    bad = np.flatnonzero(got["labels"] != ref["labels"])
    assert bad.size == 0, f"{where}: {bad.size} labels differ, first rows {bad[:8]}"
    assert np.array_equal(got["centers"], ref["centers"]), f"{where}: centres differ"
    assert got["inertia"] == ref["inertia"], f"{where}: inertia {got['inertia']} != {ref['inertia']}"
    # the engine counts changed statistic words, the oracle changed labels: zero together
    np.testing.assert_array_equal(got["changed"] > 0, np.asarray(ref["changed"], dtype=np.int64) > 0)
    np.testing.assert_array_equal(got["shift"], np.array([h["shift"] for h in ref["history"]], dtype=np.float64))


def _assert_identical(a, b, where):
    for key in ("labels", "centers", "changed", "shift"):
        assert np.array_equal(a[key], b[key]), f"{where}: {key} differs between PCM_FAST=1 and 0"
    assert a["n_iter"] == b["n_iter"] and a["inertia"] == b["inertia"], where


def _both(pcm, monkeypatch, X, C0, iters, ref, where, dtype=torch.float32, check=None):
    monkeypatch.delenv("PCM_FAST", raising=False)
    fast = _fit(pcm, X, C0, iters, dtype, check)
    monkeypatch.setenv("PCM_FAST", "0")
    slow = _fit(pcm, X, C0, iters, dtype)
    _assert_oracle(fast, ref, where + " (lean rounds)")
    _assert_oracle(slow, ref, where + " (PCM_FAST=0)")
    _assert_identical(fast, slow, where)


@pytest.mark.parametrize("name", list(CASES))
def test_lean_rounds_bitwise(pcm, name, monkeypatch):
    _, k, cap, iters, comp, cells = CASES[name]
    X, counts, C0, ref = _case(name)
    if cap is None:
        monkeypatch.delenv("PCM_TILE_CAP", raising=False)
        cap = 4096
    else:
        monkeypatch.setenv("PCM_TILE_CAP", str(cap))
    monkeypatch.setenv("PCM_CELL_TARGET", str(counts.size if counts is not None else cells))

    def check(eng):
        assert ",8," in eng.assign_kernel().replace(" ", ""), eng.assign_kernel()   # the 8-slot instance has the lean rounds
        info = eng.layout_info()
        if counts is not None:       # the engine's cells are the builder's: the tiles are the intended ones
            assert info["ncells"] == counts.size, info
            assert info["ntiles"] == int(np.sum((counts + cap - 1) // cap)), info
        st = eng.candidate_stats()
        z = eng.stream_bytes()["compressed_points"]
        print(f"{name}: {info} lists mean {st['mean']:.2f} max {st['max']} sole {st['sole_tiles']} compressed {z} of {eng.n}")
        assert st["full_cells"] == 0 and 1.0 < st["mean"] < 6.0 and st["max"] <= 16, st
        if comp == "all":
            assert z == eng.n, (z, eng.n)
        elif comp == "most":
            assert 0.9 * eng.n <= z, (z, eng.n)
        elif comp == "some":
            assert 0 < z < eng.n, (z, eng.n)

    _both(pcm, monkeypatch, X, C0, iters, ref, name, check=check)


def test_tile_shapes_of_the_cases():
    """The builders give what the cases are for (no GPU needed to see it, but kept beside them)."""
    _, counts, _, _ = _case("sizes")
    assert 4096 in counts and 4097 in counts and (counts < 512).sum() >= 2
    _, counts, _, _ = _case("quarter")
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    assert set(starts % 4) == {0, 1, 2, 3}           # tile starts of every residue
    assert ((counts % 512) != 0).all()                 # every cell's last tile ends mid-round
    assert (counts > 1024).any() and (counts < 512).any()


def test_list_lengths_one_to_past_the_slots(pcm, monkeypatch):
    """Seeds clustered in one corner: lists from one entry (sole tiles) to more than
    the 8 lane slots, so lean and generic rounds run in the same launch."""
    monkeypatch.setenv("PCM_TILE_CAP", "512")
    monkeypatch.setenv("PCM_CELL_TARGET", "512")
    X, counts = _box(0.5, 0.125, 8, np.random.default_rng(9).integers(100, 700, 512), 17)
    rng = np.random.default_rng(10)
    inside = np.flatnonzero((X < np.float32(0.5 + 0.125 / 8)).all(axis=1))      # cell 0
    C0 = np.concatenate([X[rng.choice(inside, 14, replace=False)], X[R.init_indices(X.shape[0], 34)]])
    iters = 3
    ref = R.lloyd_fit(X, C0, max_iter=iters, tol=0.0, fast=True, history=True)

    def check(eng):
        assert ",8," in eng.assign_kernel().replace(" ", ""), eng.assign_kernel()
        st = eng.candidate_stats()
        print(f"lengths: mean {st['mean']:.2f} max {st['max']} sole {st['sole_tiles']} of {eng.layout_info()['ntiles']}")
        assert st["max"] >= 9 and st["sole_tiles"] > 0 and 1.0 < st["mean"] < 8.0 and st["full_cells"] == 0, st
        assert eng.stream_bytes()["compressed_points"] == eng.n

    _both(pcm, monkeypatch, X, C0, iters, ref, "lengths", check=check)


@pytest.mark.parametrize("d,dt,k", [(4, "f16", 16), (2, "f32", 8)])
def test_other_formats(pcm, d, dt, k, monkeypatch):
    """fp16 D = 4 (generic rounds only: the instance keeps its registers) and fp32 D = 2 (lean rounds)."""
    monkeypatch.setenv("PCM_TILE_CAP", "512")
    X = R.splitmix_uniform(60_000, d, 21)
    if dt == "f16":
        X = X.astype(np.float16).astype(np.float32)
    C0 = X[R.init_indices(X.shape[0], k)]
    ref = R.lloyd_fit(X, C0, max_iter=5, tol=0.0, fast=True, history=True)
    _both(pcm, monkeypatch, X, C0, 5, ref, f"{dt} d={d}", dtype=torch.float16 if dt == "f16" else torch.float32)
