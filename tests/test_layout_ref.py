"""CPU: tests/layout_ref.py, the numpy restatement of the Lloyd layout, checked three ways.

1. Against slow, obviously-right code: Python loops over single points for the keys, the tiles,
   the compression records and their decoding, on clouds of a few hundred points.
2. Its grid against the library's own ``make_grid`` (the host-only debug export, no GPU needed).
3. Every named case of tests/layout_cases.py reaches the edge it is named for: a condition on
   the inputs, asserted from the reference alone, so that tests/test_gpu_layout_edges.py cannot
   pass by missing its edge.
"""
import ctypes
import math
import os

import numpy as np
import pytest

import layout_cases as LC
import layout_ref as LR


# ------------------------------------------------------------------ 1. slow code
def slow_key(x, g, sub, zlev):
    idx, half, fz = [], [], []
    for a in range(g.d):
        t = (float(x[a]) - g.lo[a]) * g.inv[a]
        v = min(max(int(math.floor(t)), 0), g.G[a] - 1)
        fr = t - v
        idx.append(v)
        half.append(1 if fr >= 0.5 else 0)
        fz.append(min(max(int(math.floor(fr * (1 << zlev))), 0), (1 << zlev) - 1))
    cell = 0
    for a in range(g.d):
        cell = cell * g.G[a] + idx[a]
    if zlev > 0:
        z = 0
        for lev in range(zlev):                             # level 1 (the half-cell) is the highest
            for a in range(g.d):
                z = z * 2 + ((fz[a] >> (zlev - 1 - lev)) & 1)
        return cell * (1 << (g.d * zlev)) + z
    if sub:
        s = 0
        for a in range(g.d):
            s = s * 2 + half[a]
        return cell * (1 << g.d) + s
    return cell


def slow_layout(p, X):
    n, d = X.shape
    keys = [slow_key(X[i], p.g, p.sub, p.zlev) for i in range(n)]
    perm = sorted(range(n), key=lambda i: (keys[i], i))
    shift = d * p.zlev if p.zlev else (d if p.sub else 0)
    cells = [keys[i] >> shift for i in perm]
    tiles, tile_off = [], [0]
    for c in range(p.ncells):
        pos = [j for j in range(n) if cells[j] == c]
        if pos:
            assert pos == list(range(pos[0], pos[-1] + 1))
            cnt = len(pos)
            nt = (cnt + p.tile_cap - 1) // p.tile_cap
            per = (cnt + nt - 1) // nt
            for t in range(nt):
                tiles.append((c, pos[0] + t * per, min(pos[0] + (t + 1) * per, pos[-1] + 1), 0))
        tile_off.append(len(tiles))
    return keys, perm, tiles, tile_off


def slow_tile_record(U, a, b):
    """(meta word, [records]) of the tile [a, b) of fp32 patterns U, point by point."""
    w, lo = [], []
    ok = True
    for ax in range(3):
        col = [int(U[i, ax]) for i in range(a, b)]
        if len({c >> 31 for c in col}) != 1:
            ok = False
        lo.append(min(col))
        w.append((max(col) - min(col)).bit_length())
        if w[-1] > 31:
            ok = False
    if w[2] == 0:
        w[2] = 1
    if sum(w) > 64:
        ok = False
    if not ok:
        return lo, 0, None
    recs = []
    for i in range(a, b):
        d0, d1, d2 = (int(U[i, ax]) - lo[ax] for ax in range(3))
        recs.append((d0 | (d1 << w[0]) | (d2 << (64 - w[2]))) & ((1 << 64) - 1))
    return lo, 0x80000000 | w[0] | (w[1] << 8) | (w[2] << 16), recs


SMALL = {
    "sub": dict(n=300, d=3, k=8, env={"PCM_CELL_TARGET": "27"}),
    "cells": dict(n=257, d=2, k=1, env={"PCM_CELL_TARGET": "50"}),
    "z2": dict(n=400, d=3, k=8, env={"PCM_CELL_TARGET": "8", "PCM_ZLEV": "2"}),
    "d4": dict(n=333, d=4, k=8, env={"PCM_CELL_TARGET": "81"}),
    "d1": dict(n=100, d=1, k=8, env={"PCM_CELL_TARGET": "7", "PCM_ZLEV": "3"}),
}


@pytest.mark.parametrize("name", list(SMALL))
def test_keys_order_and_tiles_against_loops(name):
    s = SMALL[name]
    rng = np.random.default_rng(len(name))
    X = rng.uniform(-1.0, 2.0, (s["n"], s["d"])).astype(np.float32)
    X[5] = X[6]                                             # a duplicate: the row breaks the tie
    X[7, 0] = X[:, 0].max()
    p = LR.plan(X, s["k"], s["env"])
    p.tile_cap = 4                                          # below the engine's floor: several tiles per cell here
    L = LR.build(p, X)
    keys, perm, tiles, tile_off = slow_layout(p, X)
    assert L.key.tolist() == keys
    assert L.perm.tolist() == perm
    assert L.tiles.tolist() == [list(t) for t in tiles]
    assert L.tile_off.tolist() == tile_off
    assert max(keys) < (1 << p.bits)
    assert len({t[0] for t in tiles}) < len(tiles)          # some cell has more than one tile
    xs = L.xs.reshape(-1)
    for i in (0, 1, 2, 3, 4, 5, s["n"] - 1):
        for a in range(s["d"]):
            assert xs[LR.xs_index(i, a, s["d"])] == X[perm[i], a]
    for i in range(s["n"], p.npad):
        assert all(xs[LR.xs_index(i, a, s["d"])] == 0 for a in range(s["d"]))
    Xs = X[perm]
    for t, (_, a, b, _) in enumerate(tiles):
        want = [sum(int(math.ldexp(float(Xs[i, ax]), int(p.q[ax]))) for i in range(a, b)) for ax in range(s["d"])]
        assert L.tsum[t].tolist() == want
        assert L.tbox[t, 0, : s["d"]].tolist() == Xs[a:b].min(0).tolist()
        assert L.tbox[t, 1, : s["d"]].tolist() == Xs[a:b].max(0).tolist()


def test_records_and_decoder_against_loops():
    c = LC.build("xz-widths")
    p = LR.plan(c.X, c.k, c.env)
    L = LR.build(p, c.X)
    U = np.ascontiguousarray(c.X[L.perm]).view(np.uint32)
    xz = np.zeros((p.npad + 255) // 256 * 512, np.uint32)
    seen = set()
    for t, (_, a, b, _) in enumerate(L.tiles.tolist()):
        lo, meta, recs = slow_tile_record(U, a, b)
        assert L.tmeta[t].tolist() == lo + [meta]
        assert bool(L.comp[t]) == (recs is not None)
        seen.add(sum((meta >> s) & 0xff for s in (0, 8, 16)) if meta else -1)
        if recs is not None:
            assert L.rec[a:b].tolist() == recs
            for i, r in zip(range(a, b), recs):
                xz[(i // 256) * 512 + i % 256] = r & 0xffffffff
                xz[(i // 256) * 512 + i % 256 + 256] = r >> 32
    assert {64, -1} <= seen
    pos, pat = LR.decode(L.tmeta, xz, L.tiles)
    assert len(pos) == L.compressed_points > 0
    np.testing.assert_array_equal(pat, U[pos])


def test_bit_length_and_llround():
    v = np.asarray([0, 1, 2, 3, 4, 255, 256, (1 << 31) - 1, 1 << 31, (1 << 32) - 1], np.uint64)
    assert LR.bit_length(v).tolist() == [int(x).bit_length() for x in v]
    assert [LR.llround(x) for x in (0.0, 0.49999999999999994, 0.5, 1.5, 2.5, 2.4999, 4095.5)] == [0, 0, 1, 2, 3, 2, 4096]


# ------------------------------------------------------------------ 2. the grid against the library
@pytest.fixture(scope="module")
def native_grid():
    from pcm_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    lib = _lib.load(require_gpu_runtime=False)
    f = lib.pcm_debug_make_grid
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                  ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]
    f.restype = ctypes.c_int

    def grid(d, lo, hi, target):
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        G = np.zeros(4, np.int32)
        nc, prune = ctypes.c_int64(), ctypes.c_int()
        assert f(d, lo.ctypes.data, hi.ctypes.data, float(target), G.ctypes.data, ctypes.byref(nc),
                 ctypes.byref(prune)) == 0
        return G[:d].tolist(), nc.value, prune.value
    return grid


BOXES = {
    "cubic": ([0, 0, 0], [1, 1, 1]),
    "offset": ([-3.5, 2.25, 100.0], [4.0, 2.75, 164.0]),
    "thin": ([0, 0, 0], [1, 1, 1e-6]),                      # far more cells than the target: the 2^20 halving
    "sliver": ([0, 0], [1000.0, 1e-3]),
    "thin4": ([0, 0, 0, 0], [1, 1, 1, 1e-9]),
    "flat-axis": ([0, 5, 0], [2, 5, 1]),                    # a degenerate axis gets one cell
    "two-flat": ([1, 1, 1, 1], [1, 9, 1, 1]),
    "constant": ([0.375] * 3, [0.375] * 3),
    "line": ([0], [1]),
    "huge": ([0, 0, 0], [2e18, 1e18, 1e18]),                # no pruning
    "fp32-box": ([float(np.float32(0.1))] * 3, [float(np.float32(0.7)), float(np.float32(0.9)), 1.0]),
}
TARGETS = (0.0, 0.3, 1.0, 2.0, 7.5, 64.0, 1000.0, 4096.0, 32768.0, 262144.0, 262145.0, 1e7)


@pytest.mark.parametrize("box", list(BOXES))
def test_grid_equals_make_grid(native_grid, box):
    lo, hi = BOXES[box]
    d = len(lo)
    halved = False
    for target in TARGETS:
        g = LR.make_grid(d, lo, hi, target)
        assert (g.G, g.ncells, g.prune) == native_grid(d, lo, hi, target), (box, target)
        assert g.ncells <= 1 << 20
        halved |= box.startswith("thin") and g.ncells > 1 << 18
    assert halved == box.startswith("thin")                 # the thin boxes do reach the halving loop
    if box in ("constant",):
        assert g.G == [1] * d
    if box == "huge":
        assert g.prune == 0


def test_cell_target_rule():
    assert LR.cell_target(28_000_000, 3, 1000) == 10_000.0                    # points per cell
    assert LR.cell_target(28_000_000, 3, 100) == 3200.0                       # 32 cells per centre
    assert LR.cell_target(10_000_000, 4, 100) == 4800.0                       # D = 4: 48 per centre, 1000 points per cell
    assert LR.cell_target(1_000_000, 4, 100) == 1000.0
    assert LR.cell_target(1_000_000, 3, 100, n_global=8_000_000) == min(400.0, 1_000_000 / 2800.0)   # a shard's share
    assert LR.cell_target(5, 3, 100, env={"PCM_CELL_TARGET": "77"}) == 77.0


# ------------------------------------------------------------------ 3. every case reaches its edge
def _plan(name):
    c = LC.build(name)
    return c, LR.plan(c.X, c.k, c.env)


def _layout(name):
    c, p = _plan(name)
    return c, p, LR.build(p, c.X)


def test_case_names_are_unique_and_buildable():
    names = LC.names() + list(LC.SEG_NAMES)
    assert len(set(names)) == len(names)
    for dt, d, ch in (("f32", 3, 4096), ("f32", 4, 3072), ("f16", 3, 4096), ("f16", 4, 4096), ("f32", 1, 4096)):
        assert LR.chunk_items(LC.DTYPES[dt], d) == ch


@pytest.mark.parametrize("name", LC.edge_names() + LC.vec_names())
def test_edge_cases_reach_their_chunks(name):
    c, p = _plan(name)
    assert c.dtype == (name.split("-")[1][:3] if name.startswith("edge") else "f32")
    assert p.nblk == -(-c.n // p.ch) and p.nseg == 1
    if c.n > 512:                                           # a real box: two passes, position maps
        assert p.npass == 2 and p.has_dmap and p.widths == [p.wb, p.bits - p.wb]
        L = LR.build(p, c.X)
        assert len(np.unique(L.key & ((1 << p.wb) - 1))) > 8 and len(np.unique(L.key >> p.wb)) > 8
    if name.startswith("vec"):
        assert c.d == 3 and c.n % 4 == int(name[-1]) % 4 and p.nblk == 5 - (c.n % 4 == 0)


PASS_WANT = {8: (1, [8], 1, 0), 9: (2, [5, 4], 1, 1), 16: (2, [8, 8], 0, 1), 17: (3, [6, 6, 5], 0, 0),
             21: (3, [7, 7, 7], 1, 0), 32: (4, [8, 8, 8, 8], 0, 0)}


@pytest.mark.parametrize("bits", LC.PASS_BITS)
def test_pass_cases_reach_their_widths(bits):
    c, p, L = _layout(f"pass-b{bits}")
    npass, widths, sub, dmap = PASS_WANT[bits]
    assert (p.bits, p.npass, p.widths, p.sub, p.has_dmap) == (bits, npass, widths, sub, dmap)
    assert 20000 <= c.n <= 50000 and p.nblk > 1
    assert (p.zlev > 0) == (bits == 32) and (bits != 21 or p.ncells == 1 << 18)
    for q in range(npass):                                  # every pass sees many digits, the top one included
        dig = (L.key >> (q * p.wb)) & ((1 << widths[q]) - 1)
        assert len(np.unique(dig)) > (1 << widths[q]) // 2
    assert int(L.key.max()).bit_length() == bits


@pytest.mark.parametrize("name", LC.SEG_NAMES)
def test_segment_cases_reach_their_segments(name):
    c, p = _plan(name)
    want = {"seg-f32d3-n1048575": (256, 1), "seg-f32d3-n1048577": (257, 2), "seg-f32d4-n786433": (257, 2),
            "seg-f32d1-n8388613": (2049, 9)}[name]
    assert (p.nblk, p.nseg) == want and p.npass == 2 and p.has_dmap
    # the extremes in the last two rows; every cloud is long enough for the box kernel's 4-row unrolled
    # loop (rows past 3 * 1024 * 256), and the D = 4 cloud's last row is the only fourth row there is
    assert (c.X[-1] == c.X.max(0)).all() and (c.X[-2] == c.X.min(0)).all()
    assert (c.X[:-2].max(0) < c.X[-1]).all() and (c.X[:-2].min(0) > c.X[-2]).all()
    assert c.n > 3 * 1024 * 256 and (name != "seg-f32d4-n786433" or c.n - 1 == 3 * 1024 * 256)


def test_skew_cases():
    for name in LC.SKEW_NAMES:
        c, p, L = _layout(name)
        cells = np.diff(L.cell_start)
        kind = name.split("-")[1]
        assert p.nblk == 4 and c.n % 4 == 1
        if kind == "onecell":
            assert p.ncells == 64 and cells.max() == c.n - 2 and (cells > 0).sum() == 3
        elif kind == "constant":
            assert p.ncells == 1 and p.g.inv == [0.0] * 3 and (L.key == 0).all() and (L.perm == np.arange(c.n)).all()
        elif kind == "alternate":
            ce = L.key >> 3
            assert set(ce[2::2]) == {0} and set(ce[3::2]) == {63}
        elif kind == "sorted":
            assert (np.diff(L.key) >= 0).all() and (L.perm == np.arange(c.n)).all()
        elif kind == "reverse":
            assert (np.diff(L.key) <= 0).all() and len(np.unique(L.key)) > 400
        elif kind == "dups":
            same = (c.X == c.X[0]).all(1)
            assert same.sum() >= 4096 and (np.diff(L.perm[np.isin(L.perm, np.flatnonzero(same))]) > 0).all()
        elif kind == "faces":
            _, fr = LR.cell_coords(c.X, p.g)
            assert p.g.G == [4, 4, 4] and p.sub and set(np.unique(fr)) == {0.0, 0.5, 1.0}
        elif kind == "digit255":
            assert p.widths == [8, 8] and p.sub == 0
            assert ((L.key & 255) == 255).mean() > 0.35 and ((L.key >> 8) == 255).mean() > 0.45


@pytest.mark.parametrize("name", ["tiles-cap512", "tiles-default"])
def test_tile_cases_reach_their_counts(name):
    c, p, L = _layout(name)
    cap = 512 if name == "tiles-cap512" else LR.TILE
    cells = np.diff(L.cell_start)
    assert p.tile_cap == cap and p.g.G == [4, 2, 2]
    for cnt, per_cell in ((0, 0), (1, 1), (cap, 1), (cap + 1, 2), (2 * cap, 2), (2 * cap + 1, 3)):
        hit = np.flatnonzero(cells == cnt)
        assert len(hit) >= 1, cnt
        assert (np.diff(L.tile_off)[hit] == per_cell).all()
    assert cells[-1] == 0 and cells[6] == 0                 # an empty last cell, and one in the middle
    assert {int(a) % 4 for a in L.tiles[:, 1]} == {0, 1, 2, 3}
    assert {int(b) % 4 for b in L.tiles[:, 2]} == {0, 1, 2, 3}
    assert ((L.tiles[:, 1] >> 8) != ((L.tiles[:, 2] - 1) >> 8)).any()          # tiles across a 256-point stream block
    assert L.comp.any() and not L.comp.all()
    assert L.ntiles == L.tile_off[-1] <= p.ntiles_cap


def test_one_cell_grid():
    c, p, L = _layout("tiles-onecell")
    assert p.ncells == 1 and L.tiles.tolist() == [[0, 0, 342, 0], [0, 342, 684, 0], [0, 684, 1025, 0]]


def _widths(L):
    m = L.tmeta[:, 3].astype(np.int64)
    return (m & 0xff) + ((m >> 8) & 0xff) + ((m >> 16) & 0xff)


def test_compression_cases():
    c, p, L = _layout("xz-widths")
    U = np.ascontiguousarray(c.X[L.perm]).view(np.uint32)
    span = np.stack([LR.bit_length(U[a:b].max(0).astype(np.int64) - U[a:b].min(0)) for _, a, b, _ in L.tiles])
    tot = span.sum(1) + (span[:, 2] == 0)
    assert p.g.G == [2, 2, 2] and L.ntiles == 6
    assert 64 in tot[L.comp] and 65 in tot[~L.comp] and (_widths(L)[L.comp] == tot[L.comp]).all()
    assert ((L.tiles[:, 2] - L.tiles[:, 1]) == 1).any()                        # a one-point tile
    assert ((span[:, 2] == 0) & L.comp).any() and ((span[:, 0] == 0) & L.comp).any()   # constant axes; z forced to a bit

    c, p, L = _layout("xz-neg")
    assert (c.X < 0).all() and L.comp.all()

    c, p, L = _layout("xz-straddle")
    Xs = c.X[L.perm]
    mixed = np.asarray([((Xs[a:b] < 0).any(0) & (Xs[a:b] >= 0).any(0)).any() for _, a, b, _ in L.tiles])
    assert mixed.any() and not L.comp[mixed].any() and L.comp.sum() >= 5 and (~L.comp & ~mixed).sum() > 20

    c, p, L = _layout("xz-zeros")
    U = np.ascontiguousarray(c.X[L.perm]).view(np.uint32)
    both = np.asarray([(U[a:b, 2] == 0).any() and (U[a:b, 2] == 0x80000000).any() for _, a, b, _ in L.tiles])
    assert both.any() and not L.comp[both].any() and L.comp.any()


def test_crowded_cases():
    c, p, L = _layout("crowd-auto")
    assert "PCM_ZLEV" not in c.env and c.k > LR.CAPF and 4 * p.tile_cap <= c.n <= 4100
    assert p.zlev == 2 and p.sub == 0 and p.bits == 6 + 3 * 2
    assert np.diff(L.cell_start).max() > 4 * p.tile_cap
    assert LR.choose_zlev(c.X, p.g, LR.CAPF, p.tile_cap, c.env) == 0           # the early exits
    assert LR.choose_zlev(c.X[:2000], p.g, c.k, p.tile_cap, c.env) == 0
    for name, z, bits in (("crowd-z1-f16d2", 1, 4 + 2), ("crowd-z3", 3, 6 + 9), ("crowd-z6", 6, 6 + 18)):
        c, p, L = _layout(name)
        assert (p.zlev, p.bits, p.sub) == (z, bits, 0)
        assert len(np.unique(L.key & ((1 << (c.d * z)) - 1))) > min(30, (1 << (c.d * z)) // 2)
        assert (np.diff(L.tile_off) > 1).any()
