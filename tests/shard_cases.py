"""Inputs of the slab sharding tests (TEST INFRASTRUCTURE ONLY; NumPy only).

One list of named cases serves tests/test_shard_ref.py (the CPU restatement of
tests/cpu_engine.py against tests/shard_ref.py) and tests/test_gpu_shard_edges.py
(the HIP operators against tests/shard_ref.py), so both are held to the same
contract on the same inputs.  A case is built on demand by ``build(name)``.

Two families:

``part-<pattern>-n<n>``  a destination pattern laid over the rows, the cloud made
    from it: row i gets the mid-point of a bin that ``owner`` gives to dest[i].
    The sizes sit on the edges of the scatter kernel (64-lane ballot, 256-row
    round, 4096-row block); the patterns are those a rank-by-ballot scatter can
    get wrong.
``bins-<kind>-b<nbins>-<dtype>``  values on and next to bin edges, at the clamp,
    below and above the range, signed zeros, denormals and values whose scaled
    coordinate is far outside int32, under a random (non-monotone) owner table.

What a case does not fix by its name (P, d, axis, dtype, bins, gidx0) is drawn
from a generator seeded by the name; tests/test_shard_ref.py asserts that the
draws cover every value together with the others it has to meet.
"""
import zlib
from types import SimpleNamespace

import numpy as np

import shard_ref as S

# constants of csrc/pcm_shard.hip the shapes rest on
WAVE, TPB, ROUNDS = 64, 256, 16
CHUNK = TPB * ROUNDS
HIST_BINS_MAX = 16384
MAXP = 16

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 77)
RANKS = (1, 2, 3, 8, 16)
RUNS = (63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
PATTERNS = ("uniform", "mod", "runs", "edges", "first", "last", "midempty", "tail", "permuted")
NBINS = (1, 2, 1000, 16384)
BIN_KINDS = ("grid", "hi", "affine", "flat", "tiny", "huge")
GIDX = ("zero", "small", "top")
DTYPES = {"f32": np.float32, "f16": np.float16}


def gidx0_of(kind, n):
    """0, a shard offset, or the largest the entry point accepts (gidx0 + n = 2^32 - 1)."""
    return {"zero": 0, "small": 12345, "top": (1 << 32) - 1 - n}[kind]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def contiguous_owner(nbins, P):
    """Monotone table, every rank owning a run of bins (what lloyd.slab_owner yields); nbins >= P."""
    return (np.arange(nbins) * P // nbins).astype(np.uint8)


def permuted_owner(nbins, P, rng):
    """A permutation of the ranks repeated over the bins: no rank's bins are contiguous."""
    return rng.permutation(P)[np.arange(nbins) % P].astype(np.uint8)


def destinations(pattern, n, P, rng):
    i = np.arange(n)
    if pattern in ("uniform", "permuted"):
        return rng.integers(0, P, n)
    if pattern == "mod":                                   # every lane of a wave differs from its neighbours
        return i % P
    if pattern == "runs":                                  # runs of 63, 64, 65, 255, ... rows, the rank changing after each
        reps = -(-max(n, 1) // sum(RUNS))
        return np.repeat(np.arange(len(RUNS) * reps) % P, np.tile(RUNS, reps))[:n]
    if pattern == "edges":                                 # the rank changes AT rows 63, 64, 65, 255, ..., 4097
        return np.searchsorted(RUNS, i, side="right") % P
    if pattern == "first":
        return np.zeros(n, np.int64)
    if pattern == "last":
        return np.full(n, P - 1)
    if pattern == "midempty":                              # P = 8, ranks 2..5 receive nothing
        return np.asarray([0, 1, 6, 7])[rng.integers(0, 4, n)]
    if pattern == "tail":                                  # only the last row goes elsewhere
        dest = np.zeros(n, np.int64)
        dest[n - 1:] = P - 1
        return dest
    raise ValueError(pattern)


def _payload_specials(X, axis):
    """-0.0 and denormals in the columns that only travel."""
    tiny = np.nextafter(X.dtype.type(0), X.dtype.type(1))
    for c in range(X.shape[1]):
        if c != axis:
            X[1::5, c] = -0.0
            X[2::5, c] = 3 * tiny
            X[3::11, c] = -tiny


def cloud_for(dest, owner, lo, inv, d, axis, dtype, rng):
    """A cloud whose row i falls in a bin that ``owner`` gives to dest[i] (the bin's mid-point)."""
    n = len(dest)
    X = rng.uniform(-4.0, 4.0, (n, d))
    b = np.zeros(n, np.int64)
    for p in np.unique(dest):
        mine = np.flatnonzero(owner == p)
        sel = dest == p
        b[sel] = mine[rng.integers(0, len(mine), int(sel.sum()))]
    X[:, axis] = lo + (b + 0.5) / inv
    X = np.ascontiguousarray(X.astype(dtype))
    _payload_specials(X, axis)
    assert np.array_equal(S.dests(X, axis, lo, inv, len(owner), owner), dest)      # the construction holds
    return X


def _case(name, X, axis, lo, inv, nbins, owner, P, gidx):
    X = np.ascontiguousarray(X)
    owner = np.ascontiguousarray(owner, dtype=np.uint8)
    assert X.ndim == 2 and owner.shape == (nbins,) and (owner < P).all() and np.isfinite(X.astype(np.float32)).all()
    return SimpleNamespace(name=name, X=X, n=X.shape[0], d=X.shape[1], axis=int(axis), lo=float(lo), inv=float(inv),
                           nbins=int(nbins), owner=owner, P=int(P), gidx=gidx, gidx0=gidx0_of(gidx, X.shape[0]),
                           dtype={np.dtype(np.float32): "f32", np.dtype(np.float16): "f16"}[X.dtype])


# ------------------------------------------------------------------ partition patterns
def part_names():
    names = [f"part-{p}-n{n}" for p in PATTERNS for n in SIZES]
    return names + [f"part-runs-n{sum(RUNS) + 77}"]        # every run of the list, whole


def _build_part(name):
    _, pattern, n = name.split("-")
    n = int(n[1:])
    rng = _rng(name)
    P = 8 if pattern == "midempty" else _pick(rng, RANKS[1:] if pattern == "tail" else RANKS)
    dtype = _pick(rng, ("f32", "f16"))
    d = _pick(rng, (1, 2, 3, 4))
    axis = int(rng.integers(0, d))
    # (lo, inv, nbins); fp16 keeps nbins <= 512 so that the bins' mid-points are representable
    lo, inv, nbins = _pick(rng, [(0.0, 16.0, 16), (0.0, 512.0, 512)] if dtype == "f16" else
                           [(0.0, 16.0, 16), (0.0, 1024.0, 1024), (0.0, 16384.0, 16384), (0.1, 1000 / 0.7, 1000)])
    owner = permuted_owner(nbins, P, rng) if pattern == "permuted" else contiguous_owner(nbins, P)
    dest = destinations(pattern, n, P, rng)
    X = cloud_for(dest, owner, lo, inv, d, axis, DTYPES[dtype], rng)
    return _case(name, X, axis, lo, inv, nbins, owner, P, _pick(rng, GIDX))


# ------------------------------------------------------------------ bin edges
def bins_names():
    return [f"bins-{k}-b{b}-{t}" for k in BIN_KINDS for b in NBINS for t in DTYPES]


def _around(e):
    """Every value, its neighbour below and its neighbour above."""
    inf = e.dtype.type(np.inf)
    return np.concatenate([e, np.nextafter(e, -inf), np.nextafter(e, inf)])


def _bin_values(kind, nbins, dtype, rng):
    """(x, lo, inv) of one kind of bin-edge input."""
    T = DTYPES[dtype]
    if kind == "grid":          # lo = 0, inv = nbins: x = b / nbins (exact for a power of two), next to it, and 1.0
        return _around((np.arange(nbins + 1) / nbins).astype(T)), 0.0, float(nbins)
    if kind == "hi":            # inv as lloyd.prepare computes it; x == hi lands on nbins and is clamped
        lo, hi = -1.25, 3.5
        x = np.concatenate([_around(np.asarray([lo, hi], T)), rng.uniform(lo, hi, 1000).astype(T)])
        return x, lo, nbins / (hi - lo)
    if kind == "affine":        # lo = 0.1, bins of 0.7 / nbins; inside, below lo, above hi, next to the edges
        lo, inv = 0.1, nbins / 0.7
        edges = (lo + rng.integers(0, nbins + 1, 1500) / inv).astype(T)
        return np.concatenate([_around(edges), rng.uniform(-0.5, 1.5, 1500).astype(T)]), lo, inv
    if kind == "flat":          # the zero-extent cloud of lloyd.prepare: inv = 0, everything in bin 0
        x = np.concatenate([rng.uniform(-100, 100, 700), [0.0, -0.0, 6e4, -6e4]]).astype(T)
        return x, float(x[0]), 0.0
    if kind == "tiny":          # -0.0 and denormals, scaled so that they spread over the bins
        e = 24 if dtype == "f16" else 140                      # j * 2^-e is a denormal up to j = 1023 / 16383
        j = np.concatenate([np.arange(-5, min(nbins, 1200) + 6), rng.integers(0, nbins + 1, 300)])
        x = np.concatenate([_around(np.ldexp(j.astype(np.float64), -e).astype(T)), np.asarray([0.0, -0.0], T)])
        return x, _pick(rng, (0.0, float(np.ldexp(3.0, -e)))), float(np.ldexp(1.0, e))
    if kind == "huge":          # (x - lo) * inv far outside int32 (and int64): the contract is the clamp
        if dtype == "f16":      # the largest fp16 values under inv = 2^40; every other value but 0 is clamped too
            big, inv = 65504.0, float(np.ldexp(1.0, 40))
            small = np.ldexp(rng.integers(-3, 4, 400).astype(np.float64), -24)
        else:                   # +-3e38 under inv = 16384, among values that spread over the bins
            big, inv = 3e38, float(HIST_BINS_MAX)
            small = rng.uniform(0, nbins / inv, 400)
        x = np.concatenate([np.asarray([big, -big] * 40), small, [0.0, -0.0]]).astype(T)
        return x, _pick(rng, (0.0, -big)), inv
    raise ValueError(kind)


def _build_bins(name):
    _, kind, nbins, dtype = name.split("-")
    nbins = int(nbins[1:])
    rng = _rng(name)
    x, lo, inv = _bin_values(kind, nbins, dtype, rng)
    x = x[rng.permutation(len(x))]
    d = _pick(rng, (1, 2, 3, 4))
    axis = int(rng.integers(0, d))
    X = rng.uniform(-4.0, 4.0, (len(x), d)).astype(DTYPES[dtype])
    _payload_specials(X, axis)
    X[:, axis] = x
    P = _pick(rng, RANKS)
    return _case(name, X, axis, lo, inv, nbins, rng.integers(0, P, nbins), P, _pick(rng, GIDX))


# ------------------------------------------------------------------ the histogram's grid-stride loop
def hist_trip(ncu):
    """Rows one trip of k_shard_hist's grid-stride loop covers: its grid is capped at 2 blocks per CU."""
    return 2 * ncu * TPB


def build_stride(ncu):
    """More than two trips of the loop (2 * trip + 333 rows, about 3 MB), every bin of the largest table in use."""
    name = "stride"
    rng = _rng(name)
    n = 2 * hist_trip(ncu) + 333
    X = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    X[:7, 1] = [1.0, 0.0, -0.0, 2.0, -1.0, np.nextafter(np.float32(1), np.float32(0)), 0.5]
    return _case(name, X, 1, 0.0, float(HIST_BINS_MAX), HIST_BINS_MAX, contiguous_owner(HIST_BINS_MAX, 16), 16, "small")


def names():
    return part_names() + bins_names()


def build(name):
    return _build_part(name) if name.startswith("part-") else _build_bins(name)
