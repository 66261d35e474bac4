"""The Lloyd engine's layout (``pcm_layout_build``) restated in numpy (TEST INFRASTRUCTURE ONLY).

Written from the documented contracts of csrc/pcm_layout.hip, pcm_layout.hpp and pcm_sort.hpp, in
fp64 and integer arithmetic, not from the kernels' loop structure: what the layout must hold, not
how the GPU gets there.  Everything it yields is an integer or a bit pattern, so the GPU is
compared with it exactly (tests/test_gpu_layout_edges.py); tests/test_layout_ref.py checks this
file itself against slow per-point loops and against the library's own ``make_grid``.

``plan(X, k, env)``   box, grid, sub / zlev, key width and the sort plan (cheap: no sort);
``build(p, X)``       keys, perm, xs, starts, tiles, tsum, compression records, tile boxes.

``env`` holds the knobs ``pcm_layout_build`` reads from the environment at every layout
(PCM_CELL_TARGET, PCM_TILE_CAP, PCM_ZLEV), as strings.
"""
import math
from types import SimpleNamespace

import numpy as np

MAXD, CAPF, TPB, LSLOT, QBITS = 4, 64, 128, 16, 25
TILE = 32 * TPB                  # PCM_TILE_PTS
RS_SEG = 256                     # chunks per scan segment (pcm_sort.hpp)
ZCROWD = 4.0
ZHI = 256


def chunk_items(dtype, d):
    """RsCfg::CH: 4096 items per chunk while a record {T c[d]; u32 row} is <= 16 bytes, else 3072."""
    return 4096 if np.dtype(dtype).itemsize * d + 4 <= 16 else 3072


# ------------------------------------------------------------------ grid
def llround(x):
    """C llround for x >= 0: nearest, halves away from zero (x - floor(x) is exact)."""
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def make_grid(d, lo, hi, target):
    """pcm::make_grid: G[], ncells, prune and the binning scale of a roughly cubic grid."""
    target = max(1.0, min(float(target), float(1 << 18)))
    ext = [float(hi[a]) - float(lo[a]) for a in range(d)]
    vol, nondeg = 1.0, 0
    for e in ext:
        if e > 0:
            vol *= e
            nondeg += 1
    G = [1] * d
    if nondeg:
        sz = math.pow(vol / target, 1.0 / nondeg)
        for a in range(d):
            if ext[a] > 0:
                G[a] = max(1, min(llround(ext[a] / sz), 4096))
    while math.prod(G) > (1 << 20):
        amax = max(range(d), key=lambda a: (G[a], -a))      # the first of the largest
        G[amax] = max(1, G[amax] // 2)
    inv = [G[a] / ext[a] if ext[a] > 0 else 0.0 for a in range(d)]
    return SimpleNamespace(d=d, G=G, ncells=math.prod(G), prune=1 if max(ext) < 1e18 else 0,
                           lo=[float(v) for v in lo[:d]], inv=inv, ext=ext)


def cell_target(n, d, k, n_global=None, env=None):
    """choose_grid's target: min(per-centre cells of this shard's share, points per cell), or PCM_CELL_TARGET."""
    ov = (env or {}).get("PCM_CELL_TARGET")
    if ov is not None:
        return float(ov)
    ng = n if n_global is None else n_global
    share = min(1.0, n / ng) if ng > 0 else 1.0
    return min((48.0 if d >= 4 else 32.0) * k * share, n / (1000.0 if d >= 4 else 2800.0))


def cell_bits(nc):
    return max(0, (int(nc) - 1).bit_length())


# ------------------------------------------------------------------ keys
def cell_coords(X, g):
    """(idx, fr): clamped cell index per axis and the fp64 position inside the cell, t - idx."""
    t = (X.astype(np.float64) - np.asarray(g.lo)[None, :]) * np.asarray(g.inv)[None, :]
    idx = np.clip(np.floor(t), 0, np.asarray(g.G)[None, :] - 1).astype(np.int64)
    return idx, t - idx


def encode(idx, G):
    c = np.zeros(idx.shape[0], np.int64)
    for a in range(len(G)):
        c = c * G[a] + idx[:, a]
    return c


def sort_keys(X, g, sub, zlev):
    """sort_key_f of every row: cell << d | half-cell bits (axis 0 highest), or the cell followed by
    the Morton code of zlev bisections (axis 0 first within a level), or the cell alone."""
    d = g.d
    idx, fr = cell_coords(X, g)
    cell = encode(idx, g.G)
    if zlev > 0:
        fz = np.clip(np.floor(fr * float(1 << zlev)), 0, (1 << zlev) - 1).astype(np.int64)
        z = np.zeros_like(cell)
        for lev in range(zlev - 1, -1, -1):
            for a in range(d):
                z = (z << 1) | ((fz[:, a] >> lev) & 1)
        return (cell << (d * zlev)) | z
    if sub:
        s = np.zeros_like(cell)
        for a in range(d):
            s = (s << 1) | (fr[:, a] >= 0.5)
        return (cell << d) | s
    return cell


# ------------------------------------------------------------------ plan
def choose_zlev(X, g, k, tile_cap, env=None):
    """The Morton levels of a crowded layout: PCM_ZLEV clamped, or from a strided occupancy sample."""
    n, d = X.shape
    zmax = min(6, (32 - cell_bits(g.ncells)) // d)
    ov = (env or {}).get("PCM_ZLEV")
    if ov is not None:
        return max(0, min(zmax, int(ov)))
    if not g.prune or k <= CAPF or n < ZCROWD * tile_cap or zmax < 1:
        return 0
    m = min(n, 1 << 20)
    idx, _ = cell_coords(X[np.arange(m) * (n // m)], g)
    est = float(np.bincount(encode(idx, g.G), minlength=g.ncells).max()) * float(n) / float(m)
    if est <= ZCROWD * tile_cap:
        return 0
    z = 1
    while z < zmax and math.ldexp(1.0, d * z) < 8.0 * est / tile_cap:
        z += 1
    return z


def plan(X, k, env=None, n_global=None):
    """Everything pcm_layout_build decides before it sorts (n > 0)."""
    env = env or {}
    n, d = X.shape
    Xf = X.astype(np.float32)
    lo, hi = Xf.min(0).astype(np.float64), Xf.max(0).astype(np.float64)
    g = make_grid(d, lo, hi, cell_target(n, d, k, n_global, env))
    if k <= 1:
        g.prune = 0
    ng = n if n_global is None else n_global
    share = min(1.0, n / ng) if ng > 0 else 1.0
    slots8 = bool(g.prune) and float(g.ncells) >= 8.0 * k * share          # lloyd_slots == 8
    tile_cap = min(TILE, max(4 * TPB, int(env.get("PCM_TILE_CAP", TILE))))
    sub = 1 if d <= 3 and not slots8 else 0
    zlev = choose_zlev(X, g, k, tile_cap, env)
    if zlev > 0:
        sub = 0
    nsub = g.ncells << (d if sub else 0)
    bits = cell_bits(g.ncells) + d * zlev if zlev > 0 else max(1, cell_bits(nsub))
    npass = max(1, (bits + 7) // 8)
    wb = -(-bits // npass)
    ch = chunk_items(X.dtype, d)
    nblk = max(1, -(-n // ch))
    maxabs = np.maximum(np.abs(lo), np.abs(hi))
    q = np.asarray([QBITS - (0 if m == 0.0 else math.frexp(m)[1]) for m in maxabs], np.int32)
    return SimpleNamespace(n=n, d=d, k=k, dtype=np.dtype(X.dtype), lo=lo, hi=hi, q=q, g=g, ncells=g.ncells, sub=sub,
                           zlev=zlev, nsub=nsub, tile_cap=tile_cap, bits=bits, npass=npass, wb=wb,
                           widths=[min(wb, bits - p * wb) for p in range(npass)], ch=ch, nblk=nblk,
                           nseg=-(-nblk // RS_SEG), has_dmap=int(npass == 2), npad=(n + 3) // 4 * 4 + 4,
                           ntiles_cap=g.ncells + n // tile_cap + 1,
                           use_xz=int(X.dtype == np.float32 and d == 3), label_bytes=2 if k <= 65535 else 4)


# ------------------------------------------------------------------ the sorted cloud
def xs_index(i, a, d):
    """AoSoA-4: groups of 4 consecutive points, coordinate-major inside a group."""
    return ((i >> 2) * d + a) * 4 + (i & 3)


def aosoa(Xs, npad):
    """The sorted rows as the engine's xs: d * npad values, zeros over [n, npad)."""
    n, d = Xs.shape
    P = np.zeros((npad, d), Xs.dtype)
    P[:n] = Xs
    return np.ascontiguousarray(P.reshape(npad // 4, 4, d).transpose(0, 2, 1)).reshape(-1)


def tile_table(cell_start, cap):
    """ceil(count / cap) tiles per cell, of per = ceil(count / tiles) points (the last one shorter)."""
    cnt = np.diff(cell_start)
    nt = -(-cnt // cap)
    tile_off = np.concatenate([[0], np.cumsum(nt)])
    cell = np.repeat(np.arange(len(cnt)), nt)
    t = np.arange(int(tile_off[-1])) - tile_off[cell]
    per = -(-cnt[cell] // np.maximum(nt[cell], 1))
    a = cell_start[cell] + t * per
    b = np.minimum(a + per, cell_start[cell + 1])
    return tile_off, np.stack([cell, a, b, np.zeros_like(a)], 1)


def bit_length(v):
    v = np.asarray(v, np.uint64)
    out = np.zeros(v.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = v >= (np.uint64(1) << np.uint64(s))
        out += np.where(big, s, 0)
        v = np.where(big, v >> np.uint64(s), v)
    return out + (v > 0)


def zword(i):
    """Word of point i's low record half in xz (the high half: + ZHI): blocks of 256 points."""
    return (i >> 8) * 512 + (i & 255)


def compress(U, tiles):
    """The compressed stream of fp32 D = 3 tiles.  U: (n, 3) uint32 patterns of the sorted points.
    tmeta (ntiles, 4) uint32; rec (n,) uint64 records (0 in raw tiles); comp (ntiles,) bool."""
    nt = len(tiles)
    a = tiles[:, 1]
    assert nt and (tiles[:, 2] > a).all() and (a[1:] == tiles[:-1, 2]).all()     # the tiles partition [0, n)
    mn = np.minimum.reduceat(U, a, axis=0).astype(np.int64)
    mx = np.maximum.reduceat(U, a, axis=0).astype(np.int64)
    sgn = U >> 31
    one_sign = np.minimum.reduceat(sgn, a, axis=0) == np.maximum.reduceat(sgn, a, axis=0)
    w = bit_length(mx - mn)
    ok = one_sign.all(1) & (w <= 31).all(1)
    w[:, 2] = np.maximum(w[:, 2], 1)                        # z sits at the top of the record: at least one bit
    ok &= w.sum(1) <= 64
    tmeta = np.zeros((nt, 4), np.uint32)
    tmeta[:, :3] = mn
    tmeta[:, 3] = np.where(ok, 0x80000000 | w[:, 0] | (w[:, 1] << 8) | (w[:, 2] << 16), 0)
    of = np.repeat(np.arange(nt), tiles[:, 2] - a)
    dlt = (U.astype(np.int64) - mn[of]).astype(np.uint64)
    w0, w2 = w[of, 0].astype(np.uint64), w[of, 2].astype(np.uint64)
    rec = dlt[:, 0] | (dlt[:, 1] << w0) | (dlt[:, 2] << (np.uint64(64) - w2))
    return tmeta, np.where(ok[of], rec, np.uint64(0)), ok


def decode(tmeta, xz, tiles):
    """(points, patterns): the sorted positions in compressed tiles and their fp32 patterns rebuilt
    from the stream: x = the low w0 bits, y = the next w1, z = the top w2 bits of the 8-byte record."""
    pos, out = [], []
    for t in np.flatnonzero(tmeta[:, 3] >> 31):
        i = np.arange(tiles[t, 1], tiles[t, 2])
        m = int(tmeta[t, 3])
        w0, w1, w2 = m & 0xff, (m >> 8) & 0xff, (m >> 16) & 0xff
        v = xz[zword(i)].astype(np.uint64) | (xz[zword(i) + ZHI].astype(np.uint64) << np.uint64(32))
        f = np.stack([v & np.uint64((1 << w0) - 1), (v >> np.uint64(w0)) & np.uint64((1 << w1) - 1),
                      v >> np.uint64(64 - w2)], 1)
        pos.append(i)
        out.append((f + tmeta[t, :3].astype(np.uint64)[None, :]).astype(np.uint32))
    if not pos:
        return np.zeros(0, np.int64), np.zeros((0, 3), np.uint32)
    return np.concatenate(pos), np.concatenate(out)


def to_fixed(Xf, q):
    """oracle.lloyd_ref.to_fixed: trunc(ldexp(x, q)) of fp32 values."""
    return np.ldexp(Xf.astype(np.float32), q.astype(np.int32)[None, :]).astype(np.int64)


def build(p, X):
    """The layout of plan p over the rows X."""
    n, d = X.shape
    key = sort_keys(X, p.g, p.sub, p.zlev)
    perm = np.lexsort((np.arange(n), key))                  # the (key, row) order
    ks = key[perm]
    Xs = X[perm]
    L = SimpleNamespace(key=key, perm=perm, xs=aosoa(Xs, p.npad))
    if p.zlev > 0:
        L.sub_start = None
        L.cell_start = np.searchsorted(ks >> (d * p.zlev), np.arange(p.ncells + 1))
    else:
        L.sub_start = np.searchsorted(ks, np.arange(p.nsub + 1))
        L.cell_start = L.sub_start[:: 1 << (d if p.sub else 0)]
    L.tile_off, L.tiles = tile_table(L.cell_start, p.tile_cap)
    L.ntiles = len(L.tiles)
    a = L.tiles[:, 1]
    Xf = Xs.astype(np.float32)
    L.tsum = np.add.reduceat(to_fixed(Xf, p.q), a, axis=0)
    L.tbox = np.zeros((L.ntiles, 2, 4), np.float32)
    L.tbox[:, 0, :d] = np.minimum.reduceat(Xf, a, axis=0)
    L.tbox[:, 1, :d] = np.maximum.reduceat(Xf, a, axis=0)
    if p.use_xz:
        L.tmeta, L.rec, L.comp = compress(np.ascontiguousarray(Xf).view(np.uint32), L.tiles)
        L.compressed_points = int((L.tiles[L.comp, 2] - L.tiles[L.comp, 1]).sum())
    else:
        L.compressed_points = 0
    L.stream_bytes = L.compressed_points * 8.0 + (n - L.compressed_points) * float(d * X.dtype.itemsize)
    return L
