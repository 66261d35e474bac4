"""GPU: sole-owner tiles of k_lloyd1.

A tile whose cell has a one-entry candidate list is credited to that centroid
from the tile's layout-time fixed-point sums (`tsum`) without reading its
points; the list builders keep an owner word per tile.  Every case forces a
dense grid on a small cloud (PCM_CELL_TARGET, read at every layout), first
checks that the engine reports at least a quarter of its tiles as sole-owner
tiles (otherwise the path under test was not taken; shares of the shapes below
by the 8-corner test on the CPU: 0.61 for K=8 over 12^3 cells, 0.88 for D=2,
0.39 for fp16 D=4 K=16 over 10^4 cells, 0.43 for K=4 over 6^3 cells), and then
requires the fit to equal oracle.lloyd_ref bit for bit: labels, centres, n_iter
and the exact inertia.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import lloyd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = 0.25


@pytest.fixture(scope="module")
def pcm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pcm_amd
    return pcm_amd


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """(X, C0, torch dtype name) of a named case; built once, never modified."""
    if name == "f32":
        X = R.splitmix_uniform(200_000, 3, 7)
        k = 8
    elif name == "mixed":                                   # axes straddle 0: raw tiles beside compressed ones
        X = R.splitmix_uniform(200_000, 3, 7) - np.float32(0.5)
        k = 8
    elif name == "d2":
        X = R.splitmix_uniform(200_000, 2, 7)
        k = 8
    elif name == "f16d4":                                   # sums from k_tile_sums
        X = R.splitmix_uniform(200_000, 4, 7).astype(np.float16).astype(np.float32)
        k = 16
    elif name == "multi":                                   # 6^3 cells of ~1850 points: 4 tiles of <= 512
        X = R.splitmix_uniform(400_000, 3, 7)
        k = 4
    elif name == "over":                                    # 4^3 cells of ~6250 points: 13 tiles per cell
        X = R.splitmix_uniform(400_000, 3, 7)
        k = 2
    elif name == "small":
        X = R.splitmix_uniform(50_000, 3, 7)
        k = 8
    else:
        raise KeyError(name)
    X.setflags(write=False)
    C0 = X[R.init_indices(X.shape[0], k)].copy()
    C0.setflags(write=False)
    return X, C0


@functools.lru_cache(maxsize=None)
def _ref(name, iters):
    X, C0 = _cloud(name)
    return R.lloyd_fit(X, C0, max_iter=iters, tol=0.0, fast=True)


def _dtype(name):
    return torch.float16 if name == "f16d4" else torch.float32


def _prepared(name, iters, X=None, C0=None):
    """Engine with the layout of the named cloud and a begun fit; the share floor checked."""
    from pcm_amd import lloyd
    from pcm_amd.engine import Engine
    if X is None:
        X, C0 = _cloud(name)
    eng = Engine(X.shape[1], C0.shape[0], _dtype(name), max_iter=iters)
    Xt = torch.from_numpy(np.array(X)).to("cuda", _dtype(name))
    Ct = torch.from_numpy(np.array(C0, dtype=np.float32)).cuda()
    q, _ = lloyd.prepare(eng, Xt, lloyd.LOCAL)
    eng.begin(Ct, 0.0, iters)
    return eng, Xt, Ct, q


def _share(eng):
    st = eng.candidate_stats()
    nt = eng.layout_info()["ntiles"]
    print(f"sole_tiles {st['sole_tiles']} of {nt} tiles, sole_points {st['sole_points']} of {eng.n}")
    return st, nt


def _assert_floor(eng):
    st, nt = _share(eng)
    assert st["sole_tiles"] >= FLOOR * nt, (st, nt)
    assert 0 < st["sole_points"] <= eng.n
    return st, nt


def _assert_same(res, ref, where):
    assert res.n_iter == ref["n_iter"], f"{where}: n_iter {res.n_iter} != {ref['n_iter']}"
    bad = np.flatnonzero(res.labels.cpu().numpy() != ref["labels"])
    assert bad.size == 0, f"{where}: {bad.size} labels differ, first rows {bad[:8]}"
    assert np.array_equal(res.centers.cpu().numpy(), ref["centers"]), f"{where}: centres differ"
    assert res.inertia == ref["inertia"], f"{where}: inertia {res.inertia} != {ref['inertia']}"


def _fit(pcm, eng, Xt, Ct, iters, **kw):
    res = pcm.lloyd_fit(Xt, Ct, max_iter=iters, tol=0.0, engine=eng, **kw)
    torch.cuda.synchronize()
    return res


# cells per case; "mixed": 20^3, since the 12^3 cells of [-0.5, 0.5) span too many fp32
# patterns per axis for any tile to compress (3 x 22 bits)
CELLS = {"f32": "1728", "mixed": "8000", "d2": "1728", "f16d4": "10000", "small": "1728"}


@pytest.mark.parametrize("name", ["f32", "mixed", "d2", "f16d4"])
def test_formats_bitwise(pcm, name, monkeypatch):
    monkeypatch.setenv("PCM_CELL_TARGET", CELLS[name])
    eng, Xt, Ct, _ = _prepared(name, 12)
    _assert_floor(eng)
    if name in ("f32", "mixed"):
        z = eng.stream_bytes()["compressed_points"]
        assert z > 0 and (name == "f32" or z < eng.n)        # "mixed": sign-straddling tiles stay raw
    _assert_same(_fit(pcm, eng, Xt, Ct, 12), _ref(name, 12), name)
    eng.close()


def test_one_step_statistics_exact(pcm, monkeypatch):
    """The int64 statistics of one assign step, word for word against the C oracle."""
    from oracle import cref
    monkeypatch.setenv("PCM_CELL_TARGET", "512")            # 8^3 cells (share 0.46 on the CPU)
    X, C0 = _cloud("f32")
    eng, _, _, q = _prepared("f32", 4)
    _assert_floor(eng)
    eng.iter_local()
    torch.cuda.synchronize()
    k, d = C0.shape
    got = eng.stats[: k * (d + 1)].cpu().numpy().reshape(k, d + 1)
    _, sums, counts, _ = cref.lloyd_stats(X, C0, q)
    np.testing.assert_array_equal(got[:, :d], sums)
    np.testing.assert_array_equal(got[:, d], counts)
    eng.close()


def test_several_tiles_per_cell(pcm, monkeypatch):
    """Cells of 3-4 tiles: every tile of a one-entry cell carries the owner word."""
    monkeypatch.setenv("PCM_CELL_TARGET", "216")
    monkeypatch.setenv("PCM_TILE_CAP", "512")
    eng, Xt, Ct, _ = _prepared("multi", 12)
    info = eng.layout_info()
    assert 2 * info["ncells"] < info["ntiles"] <= 4 * info["ncells"], info
    _assert_floor(eng)
    _assert_same(_fit(pcm, eng, Xt, Ct, 12), _ref("multi", 12), "multi")
    eng.close()


def test_cells_past_the_tile_bound_stream(pcm, monkeypatch):
    """Cells of more tiles than the writers' bound (8) keep the word 0: K = 2 over
    4^3 cells has one-entry lists (mean list length below 2), yet no sole tile."""
    monkeypatch.setenv("PCM_CELL_TARGET", "64")
    monkeypatch.setenv("PCM_TILE_CAP", "512")
    eng, Xt, Ct, _ = _prepared("over", 8)
    info = eng.layout_info()
    assert info["ntiles"] > 8 * info["ncells"], info
    st, _ = _share(eng)
    assert st["mean"] < 2.0 and st["full_cells"] == 0, st
    assert st["sole_tiles"] == 0 and st["sole_points"] == 0, st
    _assert_same(_fit(pcm, eng, Xt, Ct, 8), _ref("over", 8), "over")
    eng.close()


def test_stale_words_second_begin(pcm, monkeypatch):
    """One engine and layout, two fits from different centres: the second fit's
    lists rewrite every owner word of the first."""
    from pcm_amd import lloyd
    monkeypatch.setenv("PCM_CELL_TARGET", "1728")
    X, C0a = _cloud("f32")
    n, k = X.shape[0], C0a.shape[0]
    C0b = X[(R.init_indices(n, k) + n // (2 * k)) % n].copy()
    eng, Xt, Ct, _ = _prepared("f32", 12)
    _assert_floor(eng)
    lloyd.run(eng, Ct, 12, 0.0, lloyd.LOCAL)
    Cb = torch.from_numpy(C0b).cuda()
    st, _ = lloyd.run(eng, Cb, 12, 0.0, lloyd.LOCAL)
    labels, centers, inertia = lloyd.finish(eng, lloyd.LOCAL)
    torch.cuda.synchronize()
    ref = R.lloyd_fit(X, C0b, max_iter=12, tol=0.0, fast=True)
    assert int(st["iter"]) == ref["n_iter"]
    np.testing.assert_array_equal(labels.cpu().numpy(), ref["labels"])
    np.testing.assert_array_equal(centers.cpu().numpy(), ref["centers"])
    assert inertia == ref["inertia"]
    eng.close()


def test_stale_words_relocation(pcm, monkeypatch):
    """Empty clusters on the dense grid: halt, relocation, resume (k_cand rebuilds the lists)."""
    monkeypatch.setenv("PCM_CELL_TARGET", "1728")
    X = R.splitmix_uniform(100_000, 3, 13)
    far = np.full((6, 3), 500.0, dtype=np.float32) + np.arange(6, dtype=np.float32)[:, None]
    C0 = np.concatenate([X[:10], far])                      # 6 empty clusters on the first step
    eng, Xt, Ct, _ = _prepared("reloc", 20, X, C0)
    _assert_floor(eng)
    res = _fit(pcm, eng, Xt, Ct, 20, chunk=3)
    assert res.relocations >= 1
    _assert_same(res, R.lloyd_fit(X, C0, max_iter=20, tol=0.0, fast=True), "reloc")
    eng.close()


def test_stale_words_refresh_to_convergence(pcm, monkeypatch):
    """A fit run to convergence: most iterations refresh the lists (drift budget)
    and leave the owner words as the last rebuild wrote them."""
    monkeypatch.setenv("PCM_CELL_TARGET", "1728")
    eng, Xt, Ct, _ = _prepared("small", 80)
    _assert_floor(eng)
    res = _fit(pcm, eng, Xt, Ct, 80)
    rebuilds = eng.status()["list_rebuilds"]
    print(f"n_iter {res.n_iter}, list rebuilds {rebuilds}")
    assert rebuilds < res.n_iter, (rebuilds, res.n_iter)
    _assert_same(res, _ref("small", 80), "small")
    eng.close()


def test_stale_words_follow_reordered_tiles(pcm, monkeypatch):
    """PCM_TILE_LPT=1: the tiles are reordered at every fit start; words and sums follow."""
    monkeypatch.setenv("PCM_CELL_TARGET", "1728")
    monkeypatch.setenv("PCM_TILE_LPT", "1")
    eng, Xt, Ct, _ = _prepared("f32", 12)                   # first reorder
    _assert_floor(eng)
    eng.begin(Ct, 0.0, 12)                                  # a reorder of reordered tiles
    _assert_floor(eng)
    _assert_same(_fit(pcm, eng, Xt, Ct, 12), _ref("f32", 12), "lpt")
    eng.close()


def test_stale_words_unfused_update(pcm, monkeypatch):
    """PCM_FUSED_UPD=0: k_upd1 + k_lists write the owner words."""
    monkeypatch.setenv("PCM_CELL_TARGET", "1728")
    monkeypatch.setenv("PCM_FUSED_UPD", "0")
    eng, Xt, Ct, _ = _prepared("f32", 12)
    _assert_floor(eng)
    _assert_same(_fit(pcm, eng, Xt, Ct, 12), _ref("f32", 12), "unfused")
    eng.close()


def test_graph_replay(pcm, monkeypatch):
    """iterate(4) captured once and replayed three times equals the eager fit and the oracle."""
    from pcm_amd import lloyd
    monkeypatch.setenv("PCM_CELL_TARGET", "1728")
    ref = _ref("f32", 12)
    eng, Xt, Ct, _ = _prepared("f32", 12)
    _assert_floor(eng)
    eager = _fit(pcm, eng, Xt, Ct, 12)
    _assert_same(eager, ref, "eager")
    eng.begin(Ct, 0.0, 12)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.iterate(4)
    for _ in range(3):
        graph.replay()
    labels, centers, inertia = lloyd.finish(eng, lloyd.LOCAL)
    torch.cuda.synchronize()
    assert eng.status()["iter"] == ref["n_iter"]
    assert torch.equal(centers, eager.centers) and torch.equal(labels, eager.labels)
    np.testing.assert_array_equal(centers.cpu().numpy(), ref["centers"])
    np.testing.assert_array_equal(labels.cpu().numpy(), ref["labels"])
    assert inertia == ref["inertia"]
    del graph
    eng.close()


def test_knob_off(pcm, monkeypatch):
    """PCM_SOLE=0: no owner word is set, the result is the same."""
    monkeypatch.setenv("PCM_CELL_TARGET", "1728")
    monkeypatch.setenv("PCM_SOLE", "0")
    eng, Xt, Ct, _ = _prepared("f32", 12)
    st, _ = _share(eng)
    assert st["sole_tiles"] == 0 and st["sole_points"] == 0, st
    _assert_same(_fit(pcm, eng, Xt, Ct, 12), _ref("f32", 12), "knob off")
    eng.close()
