"""NumPy reference of ``pcm_height_grid`` (TEST INFRASTRUCTURE ONLY).

``encode`` builds the words exactly as include/pcm_kmeans.h lays them out:
float32 pixel arithmetic (one rounded subtraction, ``np.ldexp``, ``np.floor``,
compared as floats), ``zq = trunc(ldexp(z, q))``, then ``np.add.at`` and
``np.maximum.at`` on uint64 planes.
"""
import numpy as np

BIAS = 1 << 25
LOW = 0xFFFFFFFF


def fixed_q(z):
    """The default exponent of ``height_grid``: ``fixed_q([max|z|])[0]``."""
    m = float(np.max(np.abs(z))) if np.size(z) else 0.0
    return 25 - (0 if m == 0.0 else int(np.frexp(m)[1]))


def encode(X, shape, q, *, origin=(0.0, 0.0), s=0, labels=None, k=1, groups=None, n_groups=1):
    """uint64 words (G, 4, H, W), and the counts (outside, skipped)."""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    n = X.shape[0]
    H, W = int(shape[0]), int(shape[1])
    G = int(n_groups)
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    g = np.zeros(n, np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    z, y, x = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        zt = np.trunc(np.ldexp(z, np.int32(q)))                                   # float32
        fy = np.floor(np.ldexp(y - np.float32(origin[0]), np.int32(-s)))
        fx = np.floor(np.ldexp(x - np.float32(origin[1]), np.int32(-s)))
        assert zt.dtype == fy.dtype == fx.dtype == np.float32
        valid = np.isfinite(X).all(axis=1) & (lab >= 0) & (lab < k) & (g >= 0) & (g < G) & (np.abs(zt) < np.float32(BIAS))
        inside = valid & (fy >= 0) & (fy < np.float32(H)) & (fx >= 0) & (fx < np.float32(W))
    out = np.zeros((G, 4, H * W), np.uint64)
    zq = zt[inside].astype(np.int64)
    gi = g[inside]
    pix = fy[inside].astype(np.int64) * W + fx[inside].astype(np.int64)
    low = (LOW - lab[inside]).astype(np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(out[:, 0], (gi, pix), np.uint64(1))
        np.add.at(out[:, 1], (gi, pix), zq.view(np.uint64))
    np.maximum.at(out[:, 2], (gi, pix), ((zq + BIAS).astype(np.uint64) << np.uint64(32)) | low)
    np.maximum.at(out[:, 3], (gi, pix), ((BIAS - zq).astype(np.uint64) << np.uint64(32)) | low)
    return out.reshape(G, 4, H, W), (int(np.count_nonzero(valid & ~inside)), int(n - np.count_nonzero(valid)))


def direct(X, shape, q, *, origin=(0.0, 0.0), s=0, labels=None, groups=None, n_groups=1):
    """Row by row in Python: per (g, fy, fx) the list of (zq, label) of the inside rows (finite, in-range input)."""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    cells = {}
    for i, (z, y, x) in enumerate(X):
        fy = np.floor(np.ldexp(np.float32(y - np.float32(origin[0])), -s))
        fx = np.floor(np.ldexp(np.float32(x - np.float32(origin[1])), -s))
        if not (0 <= fy < shape[0] and 0 <= fx < shape[1]):
            continue
        key = (0 if groups is None else int(groups[i]), int(fy), int(fx))
        cells.setdefault(key, []).append((int(np.ldexp(z, q)), 0 if labels is None else int(labels[i])))
    return cells
