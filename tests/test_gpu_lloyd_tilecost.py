"""GPU: the fixed cost a tile pays outside its rounds in k_lloyd1.

Three things changed there and none may change a result: only the slot rows
that the fold reads are zeroed (16-byte stores, never the junk slot); the fold
reads four words per thread, sums their 16-bit halves in int32 and reduces them
over the 16-lane DPP row; and a wave takes only the rounds in which it has a
point of the tile (the upper wave owns none of a last round of a few dozen
points, and no round at all of a tile below 256 points).  Every fit here is
compared bit for bit with oracle.lloyd_ref (labels, centres, n_iter, the shift
history, the iterations at which the statistics stopped changing, the exact
inertia) and with the same fit under PCM_TILECOST=0, where every wave computes
every round.

The clouds are built cell by cell (`_cloud`, as tests/test_gpu_lloyd_fastpath.py
does), one tile per cell, in the engine's cell order, so a tile's start and end
are the running sums of the cell populations; the layout's cell and tile counts
are asserted.  A round is 512 points from base0 = start & ~3, so the points of
a tile's last round are (end - base0) mod 512.

The engine reports the mean and the longest candidate list and the sole-owner
tiles, not a histogram.  `lists` therefore places its seeds so that the number
of distinct winners per cell -- a lower bound of the cell's list, computed
here on the CPU -- takes the values 1, 2, 3, 8, 9 and 17 among others, and
asserts the longest list (>= 17: slot map and int64 overflow words beside the
lean rounds in one launch) and the sole tiles on the engine.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import lloyd_ref as R  # noqa: E402

ROUND = 512
LAST_ROUNDS = (1, 255, 256, 257, 511, 512)


def _cloud(lo, size, G, counts, seed, urange=None):
    """counts[c] points in cell c (row-major) of the cube [lo, lo + size)^3 cut into
    G^3 cells, the cube's two corners among them (they pin the engine's bounding
    box, so its grid is this one).  Points lie in the fraction urange[c] (default
    (0.1, 0.9)) of their cell along every axis.  Returns the shuffled rows and the
    cell of each row."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64).copy()
    assert counts.size == G ** 3 and counts.min() >= 1 and counts[0] >= 2 and counts[-1] >= 2
    counts[0] -= 1
    counts[-1] -= 1
    cell = np.repeat(np.arange(G ** 3), counts)
    idx = np.stack([cell // (G * G), (cell // G) % G, cell % G], axis=1).astype(np.float64)
    ulo = np.full(G ** 3, 0.1)
    uhi = np.full(G ** 3, 0.9)
    for c, (a, b) in (urange or {}).items():
        ulo[c], uhi[c] = a, b
    u = ulo[cell, None] + (uhi - ulo)[cell, None] * rng.random((cell.size, 3))
    X = lo + (idx + u) * (size / G)
    corners = np.array([[lo] * 3, [lo + size * (1 - 1e-4)] * 3])
    X = np.concatenate([X, corners]).astype(np.float32)
    cell = np.concatenate([cell, [0, G ** 3 - 1]])
    p = rng.permutation(X.shape[0])
    return X[p], cell[p]


def _tile_spans(counts):
    """(start, end) of every cell's tile: cells are laid out in cell order, one tile each."""
    ends = np.cumsum(np.asarray(counts, dtype=np.int64))
    return ends - counts, ends


def _last_round(start, end):
    n = (end - (start & ~3)) % ROUND
    return np.where(n == 0, ROUND, n)


def _round_counts():
    """64 cell populations: last rounds of every size in LAST_ROUNDS at one to four rounds
    per tile, starts of every residue mod 4, tiles below 256 points and one of exactly 4096."""
    special = {7: 4096, 20: 100, 33: 255, 46: 37, 59: 3}
    counts, s = [], 0
    for c in range(64):
        if c in special:
            n = special[c]
        else:
            n = ROUND * ((c // 6) % 4) + LAST_ROUNDS[c % 6] - (s & 3)
            if n < 2:
                n += ROUND
        counts.append(n)
        s += n
    return np.array(counts, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _rounds_case():
    """[-1, 0.75)^3, 4^3 cells: both signs, the third cell of every axis straddles 0."""
    counts = _round_counts()
    X, _ = _cloud(-1.0, 1.75, 4, counts, 31)
    X.setflags(write=False)
    C0 = X[R.init_indices(X.shape[0], 8)].copy()
    return X, counts, C0


@functools.lru_cache(maxsize=None)
def _rounds_ref():
    X, _, C0 = _rounds_case()
    return R.lloyd_fit(X, C0, max_iter=5, tol=0.0, fast=True, history=True)


LIST_G = 8
LIST_LO, LIST_SIZE = -0.9995, 1.999
# cell (ix, iy, iz) -> seeds placed on points of that cell
LIST_SEEDS = {(1, 1, 1): 17, (1, 4, 2): 9, (2, 2, 5): 8, (1, 6, 6): 3, (3, 5, 1): 2}
LIST_LONE = (5, 3, 3)      # one seed at this cell's centre, nothing else near: sole-owner tiles around it


def _cid(c):
    return (c[0] * LIST_G + c[1]) * LIST_G + c[2]


@functools.lru_cache(maxsize=None)
def _lists_case():
    """[-0.9995, 0.9995)^3, 8^3 cells.  The two corner cells hold exactly 4096 points each, packed
    into the outermost tenth of the cube (|x| in (0.964, 0.9995) on every axis: q = 25,
    |xq| just under 2^25), with one seed in the pack and a second one at the cell's far
    end that wins none of them: the tile is streamed (two candidates), all its points
    land in one slot, so every coordinate word sums 64 values of one sign near 2^25
    (about -+2^31 * 0.98) and every count word reaches 64."""
    G = LIST_G
    rng = np.random.default_rng(41)
    counts = rng.integers(200, 1100, G ** 3)
    counts[(counts % ROUND) == 0] += 1
    last = G ** 3 - 1
    counts[0] = counts[last] = 4096
    ur = {0: (0.02, 0.14), last: (0.86, 0.996)}
    X, cell = _cloud(LIST_LO, LIST_SIZE, G, counts, 42, ur)
    w = LIST_SIZE / G
    seeds = []
    for c, m in LIST_SEEDS.items():
        rows = np.flatnonzero(cell == _cid(c))
        seeds.append(X[rng.choice(rows, m, replace=False)])
    seeds.append((LIST_LO + (np.array(LIST_LONE) + 0.5) * w)[None, :].astype(np.float32))
    for c, inner in ((0, 0.95), (last, 0.05)):
        rows = np.flatnonzero(cell == c)
        ctr = X[rows].astype(np.float64).mean(axis=0)
        seeds.append(X[rows[np.argmin(((X[rows] - ctr) ** 2).sum(axis=1))]][None, :])
        ci = np.array([c // (G * G), (c // G) % G, c % G])
        seeds.append((LIST_LO + (ci + inner) * w)[None, :].astype(np.float32))
    C0 = np.concatenate(seeds).astype(np.float32)
    X.setflags(write=False)
    return X, cell, counts, C0


@functools.lru_cache(maxsize=None)
def _lists_ref():
    X, _, _, C0 = _lists_case()
    return R.lloyd_fit(X, C0, max_iter=3, tol=0.0, fast=True, history=True)


def test_round_shapes():
    """The builder gives the tiles the rounds case is for (no GPU needed)."""
    counts = _round_counts()
    start, end = _tile_spans(counts)
    assert counts.max() == 4096 and (counts == 4096).sum() == 1 and (counts < 256).sum() >= 4
    assert set(start % 4) == {0, 1, 2, 3}
    lr = _last_round(start, end)
    big = counts >= 256
    assert set(LAST_ROUNDS) <= set(lr[big].tolist()), sorted(set(lr.tolist()))
    for n in LAST_ROUNDS:      # at every size: a tile of several rounds
        assert (counts[lr == n] > ROUND).any(), n
    # the upper wave owns nothing of a last round of <= 256 points (less the lanes before `start`)
    assert ((lr <= 256) & (counts > ROUND)).sum() >= 8


def test_list_shapes():
    """Distinct winners per cell (a lower bound of its candidate list) and the corner tiles' words."""
    X, cell, counts, C0 = _lists_case()
    assert C0.shape[0] * 8 <= LIST_G ** 3          # the 8-slot instance
    lab = R.assign(np.asarray(X), C0)
    nw = np.array([np.unique(lab[cell == c]).size for c in range(LIST_G ** 3)])
    assert {1, 2, 3, 8, 9, 17} <= set(nw.tolist()), sorted(set(nw.tolist()))
    q = R.fixed_q(np.asarray(X))
    xq = R.to_fixed(np.asarray(X), q)
    for c, sign in ((0, -1), (LIST_G ** 3 - 1, 1)):
        rows = cell == c
        assert rows.sum() == 4096 and np.unique(lab[rows]).size == 1            # one slot takes the whole tile
        v = xq[rows].astype(np.int64) * sign
        assert v.min() > 0.96 * 2 ** 25 and v.max() < 2 ** 25, (v.min(), v.max())   # 64 of them: within 4 % of 2^31


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
    np.testing.assert_array_equal(got["changed"] > 0, np.asarray(ref["changed"], dtype=np.int64) > 0)
    np.testing.assert_array_equal(got["shift"], np.array([h["shift"] for h in ref["history"]], dtype=np.float64))


def _both(pcm, monkeypatch, X, C0, iters, ref, where, dtype=torch.float32, check=None):
    monkeypatch.delenv("PCM_TILECOST", raising=False)
    new = _fit(pcm, X, C0, iters, dtype, check)
    monkeypatch.setenv("PCM_TILECOST", "0")
    old = _fit(pcm, X, C0, iters, dtype)
    _assert_oracle(new, ref, where)
    _assert_oracle(old, ref, where + " (PCM_TILECOST=0)")
    for key in ("labels", "centers", "changed", "shift"):
        assert np.array_equal(new[key], old[key]), f"{where}: {key} differs between PCM_TILECOST=1 and 0"
    assert new["n_iter"] == old["n_iter"] and new["inertia"] == old["inertia"], where


@pytest.fixture(scope="module")
def pcm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pcm_amd
    return pcm_amd


@pytest.mark.gpu
def test_last_rounds_and_starts_bitwise(pcm, monkeypatch):
    X, counts, C0 = _rounds_case()
    ref = _rounds_ref()
    monkeypatch.delenv("PCM_TILE_CAP", raising=False)
    monkeypatch.setenv("PCM_CELL_TARGET", str(counts.size))

    def check(eng):
        assert ",8," in eng.assign_kernel().replace(" ", ""), eng.assign_kernel()
        info = eng.layout_info()
        assert info["ncells"] == counts.size and info["ntiles"] == counts.size, info   # one tile per cell
        st = eng.candidate_stats()
        print(f"rounds: {info} lists mean {st['mean']:.2f} max {st['max']} sole {st['sole_tiles']} "
              f"compressed {eng.stream_bytes()['compressed_points']} of {eng.n}")
        assert st["full_cells"] == 0 and st["sole_tiles"] < counts.size, st

    _both(pcm, monkeypatch, X, C0, 5, ref, "rounds", check=check)


@pytest.mark.gpu
def test_list_lengths_signs_and_counts_bitwise(pcm, monkeypatch):
    X, cell, counts, C0 = _lists_case()
    ref = _lists_ref()
    monkeypatch.delenv("PCM_TILE_CAP", raising=False)
    monkeypatch.setenv("PCM_CELL_TARGET", str(counts.size))

    def check(eng):
        assert ",8," in eng.assign_kernel().replace(" ", ""), eng.assign_kernel()
        info = eng.layout_info()
        assert info["ncells"] == counts.size and info["ntiles"] == counts.size, info
        st = eng.candidate_stats()
        print(f"lists: {info} lists mean {st['mean']:.2f} max {st['max']} sole {st['sole_tiles']} "
              f"compressed {eng.stream_bytes()['compressed_points']} of {eng.n}")
        assert st["max"] >= 17 and st["sole_tiles"] > 0 and st["full_cells"] == 0, st

    _both(pcm, monkeypatch, X, C0, 3, ref, "lists", check=check)


@pytest.mark.gpu
@pytest.mark.parametrize("d,dt,k", [(4, "f16", 16), (2, "f32", 8)])
def test_other_formats(pcm, d, dt, k, monkeypatch):
    """fp16 D = 4 (generic rounds, 16-bit points) and fp32 D = 2 (three rows per slot)."""
    monkeypatch.delenv("PCM_TILE_CAP", raising=False)
    X = R.splitmix_uniform(60_000, d, 23)
    if dt == "f16":
        X = X.astype(np.float16).astype(np.float32)
    C0 = X[R.init_indices(X.shape[0], k)]
    ref = R.lloyd_fit(X, C0, max_iter=5, tol=0.0, fast=True, history=True)
    _both(pcm, monkeypatch, X, C0, 5, ref, f"{dt} d={d}", dtype=torch.float16 if dt == "f16" else torch.float32)
