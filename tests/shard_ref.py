"""NumPy reference of the slab sharding operators (TEST INFRASTRUCTURE ONLY).

The contract of csrc/pcm_shard.hip and include/pcm_kmeans.h, written once more
from the header's words and from nothing in the package:

  bin(x)  = clip(floor((x[axis] - lo) * inv), 0, nbins - 1), in float64 from the
            exact input value (fp16 -> fp32 -> fp64 loses nothing);
  hist    = bincount of the bins;
  partition: rows grouped by ``owner[bin]`` in their original order (a stable
            sort), each with its global index ``gidx0 + i`` as a uint32 word;
  scatter_labels: ``out[rows[i] - gidx0] = labels[i]``.

Every output is an integer: comparisons with it are exact.
"""
import numpy as np


def bins(X, axis, lo, inv, nbins):
    """int64 bin of every row."""
    x = np.asarray(X)[:, axis].astype(np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.floor((x - np.float64(lo)) * np.float64(inv))
    assert not np.isnan(t).any(), "the operators are defined for finite input only"
    return np.clip(t, 0.0, float(nbins - 1)).astype(np.int64)      # clamped as a double: no cast out of range


def hist(X, axis, lo, inv, nbins):
    return np.bincount(bins(X, axis, lo, inv, nbins), minlength=nbins).astype(np.int64)


def dests(X, axis, lo, inv, nbins, owner):
    """Destination rank of every row."""
    owner = np.asarray(owner, np.int64)
    assert owner.shape == (nbins,)
    return owner[bins(X, axis, lo, inv, nbins)]


def partition(X, axis, lo, inv, nbins, owner, P, gidx0):
    """(order, rows_u32, counts): ``X[order]`` is the partitioned cloud."""
    dest = dests(X, axis, lo, inv, nbins, owner)
    assert dest.size == 0 or (0 <= dest.min() and dest.max() < P)
    order = np.argsort(dest, kind="stable")
    rows_u32 = ((order.astype(np.int64) + int(gidx0)) % (1 << 32)).astype(np.uint32)
    return order, rows_u32, np.bincount(dest, minlength=P).astype(np.int64)


def scatter_labels(labels, rows_u32, gidx0, n):
    """Labels in the partition's order -> the caller's row order (int32)."""
    at = np.asarray(rows_u32).astype(np.uint32).astype(np.int64) - int(gidx0)
    assert at.shape == (n,) and np.array_equal(np.sort(at), np.arange(n)), "rows are a permutation of gidx0 + [0, n)"
    out = np.empty(n, np.int32)
    out[at] = np.asarray(labels, np.int32)
    return out
