"""NumPy reference of ``pcm_cluster_stats`` (TEST INFRASTRUCTURE ONLY).

``encode`` builds the words exactly as include/pcm_kmeans.h lays them out --
``np.add.at`` on uint64 with the limb split ``lo = p & 0xffffffff``,
``hi = p >> 32`` (arithmetic shift, wrapping add) -- and ``decode`` turns words
back into Python-int moments.  ``direct`` forms the same moments from Python
ints without any limb, to check the recipe against.
"""
import numpy as np

from oracle import lloyd_ref as R


def words_per_row(d):
    return 1 + d + d * (d + 1)


def pairs(d):
    w = 1 + d
    for a in range(d):
        for b in range(a, d):
            yield a, b, w
            w += 2


def encode(X, labels, k, q, groups=None, n_groups=1):
    """uint64 words (G, K, W) and the number of skipped rows."""
    X = np.asarray(X)
    n, d = X.shape
    W = words_per_row(d)
    X = X.astype(np.float32)
    labels = np.asarray(labels).astype(np.int64)
    g = np.zeros(n, np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    ok = (labels >= 0) & (labels < k) & (g >= 0) & (g < n_groups) & np.isfinite(X).all(axis=1)
    out = np.zeros((n_groups * k, W), np.uint64)
    xq = R.to_fixed(X[ok], np.asarray(q, np.int32))          # int64, trunc(ldexp(x, q))
    key = g[ok] * k + labels[ok]
    with np.errstate(over="ignore"):
        np.add.at(out[:, 0], key, np.uint64(1))
        for a in range(d):
            np.add.at(out[:, 1 + a], key, xq[:, a].view(np.uint64))
        for a, b, w in pairs(d):
            p = xq[:, a] * xq[:, b]
            np.add.at(out[:, w], key, p.view(np.uint64) & np.uint64(0xFFFFFFFF))
            np.add.at(out[:, w + 1], key, (p >> np.int64(32)).view(np.uint64))
    return out.reshape(n_groups, k, W), int(n - np.count_nonzero(ok))


def decode(words, d):
    """Python ints: counts (G, K), sums (G, K, D), moments (G, K, D, D) as object arrays."""
    w = np.ascontiguousarray(words).view(np.int64)
    G, K, _ = w.shape
    counts = w[..., 0].astype(object)
    sums = w[..., 1:1 + d].astype(object)
    M = np.zeros((G, K, d, d), dtype=object)
    for a, b, i in pairs(d):
        for g in range(G):
            for j in range(K):
                lo = int(w[g, j, i]) & 0xFFFFFFFFFFFFFFFF
                hi = int(w[g, j, i + 1])
                M[g, j, a, b] = M[g, j, b, a] = lo + (hi << 32)
    return counts, sums, M


def direct(X, labels, k, q, groups=None, n_groups=1):
    """The same moments from Python-int arithmetic, no limbs (valid rows only)."""
    X = np.asarray(X).astype(np.float32)
    n, d = X.shape
    g = np.zeros(n, np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    xq = R.to_fixed(X, np.asarray(q, np.int32)).astype(object)
    counts = np.zeros((n_groups, k), dtype=object)
    sums = np.zeros((n_groups, k, d), dtype=object)
    M = np.zeros((n_groups, k, d, d), dtype=object)
    for i in range(n):
        gi, j = int(g[i]), int(labels[i])
        counts[gi, j] += 1
        sums[gi, j] += xq[i]
        M[gi, j] += np.outer(xq[i], xq[i])
    return counts, sums, M
