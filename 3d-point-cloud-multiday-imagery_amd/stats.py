"""Exact per-cluster, per-day moments of a labelled cloud, and what follows from them.

``cluster_stats`` runs ``pcm_cluster_stats`` once over ``(X, labels[, groups])``:
for every (group, cluster) the count, the fixed-point coordinate sums and the
fixed-point second moments, all exact integers (DESIGN.md §4 "Cluster
statistics").  Being integers they are additive over chunks, clouds and ranks
(``out=``, ``+``), like the fit's own statistics.  Means, covariances, per-day
offsets and the surface elements (normal, roughness, planarity) follow on the
host from O(G K) numbers.  There is no CPU fallback for the pass itself; the
accessors work on any words (device tensor or NumPy array).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from .fixed import fixed_q

_frac = np.frompyfunc(lambda a, b: float(a) / float(b) if b else float("nan"), 2, 1)


def _pairs(d: int):
    """(a, b, word) of the second moments: upper triangle, row-major, two words each."""
    w = 1 + d
    for a in range(d):
        for b in range(a, d):
            yield a, b, w
            w += 2


class ClusterStats:
    """The words of ``pcm_cluster_stats`` for G groups x K clusters in D dimensions.

    ``words``: int64 (G, K, W), W = 1 + D + D(D+1) -- a device tensor as
    ``cluster_stats`` returns it, or a NumPy array (int64 / uint64 bit patterns);
    ``q``: the fixed-point exponents the words were formed with; ``d``: D.
    """

    def __init__(self, words, q, d: int, _buf=None):
        d = int(d)
        W = _lib.stats_words(d)
        if not isinstance(words, torch.Tensor):
            words = np.ascontiguousarray(words).view(np.int64) if np.asarray(words).dtype == np.uint64 \
                else np.ascontiguousarray(words, dtype=np.int64)
        if words.ndim != 3 or words.shape[2] != W:
            raise ValueError(f"words must be (G, K, {W}) for d = {d}")
        self.words = words
        self.q = [int(v) for v in q]
        if len(self.q) != d:
            raise ValueError(f"q must hold {d} exponents")
        self.d = d
        self._buf = _buf     # device: the (G*K*W + 1) buffer `words` views; its last word counts skipped rows

    # ------------------------------------------------------------ shape
    @property
    def n_groups(self) -> int:
        return int(self.words.shape[0])

    @property
    def n_clusters(self) -> int:
        return int(self.words.shape[1])

    def numpy(self) -> np.ndarray:
        """The words on the host, int64 (G, K, W)."""
        w = self.words
        return w.cpu().numpy() if isinstance(w, torch.Tensor) else w

    def _same(self, other: "ClusterStats"):
        if not isinstance(other, ClusterStats) or tuple(other.words.shape) != tuple(self.words.shape) or \
                other.q != self.q or other.d != self.d:
            raise ValueError("ClusterStats differ in shape, d or q")

    # ------------------------------------------------------------ exact
    def counts(self) -> np.ndarray:
        return self.numpy()[..., 0].copy()

    def sums(self) -> np.ndarray:
        return self.numpy()[..., 1:1 + self.d].copy()

    def moments(self) -> np.ndarray:
        """sum xq_a xq_b as exact Python ints: object array (G, K, D, D), symmetric."""
        w = self.numpy()
        G, K, _ = w.shape
        M = np.zeros((G, K, self.d, self.d), dtype=object)
        for a, b, i in _pairs(self.d):
            lo = w[..., i].view(np.uint64).astype(object)
            hi = w[..., i + 1].astype(object)
            M[..., a, b] = M[..., b, a] = lo + hi * (1 << 32)
        return M

    def merged(self) -> "ClusterStats":
        """The sum over the groups, as a one-group ClusterStats."""
        w = self.words
        if isinstance(w, torch.Tensor):
            return ClusterStats(w.sum(0, keepdim=True), self.q, self.d)
        with np.errstate(over="ignore"):
            return ClusterStats(w.view(np.uint64).sum(0, keepdims=True, dtype=np.uint64), self.q, self.d)

    def __add__(self, other: "ClusterStats") -> "ClusterStats":
        self._same(other)
        a, b = self.words, other.words
        if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
            return ClusterStats(a + b.to(a.device), self.q, self.d)
        with np.errstate(over="ignore"):
            return ClusterStats(self.numpy().view(np.uint64) + other.numpy().view(np.uint64), self.q, self.d)

    # ------------------------------------------------------------ derived (float64)
    def means(self) -> np.ndarray:
        """float64(S) * 2^-q / float64(count); cast to float32 this is the engine's centre update."""
        n = self.counts().astype(np.float64)
        scale = np.ldexp(1.0, -np.asarray(self.q, dtype=np.int64))
        with np.errstate(divide="ignore", invalid="ignore"):
            m = (self.sums().astype(np.float64) * scale) / n[..., None]
        m[n == 0] = np.nan
        return m

    def covariances(self) -> np.ndarray:
        """Population covariance (ddof = 0), (G, K, D, D): the numerator
        n M_ab - S_a S_b is formed in exact integer arithmetic."""
        n = self.counts().astype(object)
        S = self.sums().astype(object)
        M = self.moments()
        q = np.asarray(self.q, dtype=np.int64)
        num = n[..., None, None] * M - S[..., :, None] * S[..., None, :]
        cov = _frac(num, (n * n)[..., None, None]).astype(np.float64)
        return np.ldexp(cov, -(q[:, None] + q[None, :]))

    def offsets(self, centers) -> np.ndarray:
        """means() - centers[None]: each group's mean displacement on each cluster."""
        return self.means() - np.asarray(centers, dtype=np.float64)[None]


def accumulate(X: torch.Tensor, labels: torch.Tensor, groups8: Optional[torch.Tensor], n_groups: int, k: int,
               qa: np.ndarray, buf: torch.Tensor) -> None:
    """``pcm_cluster_stats`` on checked arguments: adds the rows' words into ``buf`` (device int64,
    n_groups * k * W + 1), stream-ordered, without any synchronisation (``groups8``: uint8 or None)."""
    from .engine import _dtype_code, _ptr, _stream
    n, d = X.shape
    rc = _lib.load().pcm_cluster_stats(_ptr(X) if n else None, _dtype_code(X), n, d, _ptr(labels) if n else None,
                                       _ptr(groups8) if (groups8 is not None and n) else None, n_groups, k,
                                       qa.ctypes.data_as(ctypes.c_void_p), _ptr(buf), _stream())
    _lib.check(rc, "pcm_cluster_stats")


def cluster_stats(X: torch.Tensor, labels: torch.Tensor, n_clusters: int, *, groups: Optional[torch.Tensor] = None,
                  n_groups: Optional[int] = None, q=None, out: Optional[ClusterStats] = None) -> ClusterStats:
    """Exact moments of the rows of ``X`` (n, d), d <= 4, float32 or float16, on
    the device, per (group, label).

    ``labels``: device int32 (n,), in [0, n_clusters).  ``groups``: any integer
    device tensor (n,) with values in [0, n_groups) -- the day or cloud of each
    row (default: one group); ``n_groups`` (<= 256) defaults to ``max + 1``.
    ``q``: the fixed-point exponents, default ``fixed_q(max|X|)`` -- what
    ``lloyd_fit`` uses for the same cloud.  ``out``: an earlier result of the
    same (G, K, d, q) to accumulate into (chunked clouds, one call per day); fewer
    than 2^31 rows in all may go into one result.  Raises ValueError when rows
    were skipped (label or group out of range, NaN or Inf).
    """
    if not (isinstance(X, torch.Tensor) and X.is_cuda):
        raise _lib.PcmError("cluster_stats expects a HIP device tensor (no CPU fallback)")
    if X.dim() != 2 or not 1 <= X.shape[1] <= 4:
        raise ValueError("X must be (n, d) with 1 <= d <= 4")
    if X.dtype not in (torch.float32, torch.float16):
        raise ValueError("points dtype must be float32 or float16")
    X = X.contiguous()
    n, d = X.shape
    k = int(n_clusters)
    if k < 1:
        raise ValueError("n_clusters must be >= 1")
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int32 and
            tuple(labels.shape) == (n,)):
        raise ValueError(f"labels must be a device int32 tensor of shape ({n},)")
    labels = labels.contiguous()
    g8 = None
    if groups is not None:
        if not (isinstance(groups, torch.Tensor) and groups.is_cuda and tuple(groups.shape) == (n,)) or \
                groups.dtype.is_floating_point or groups.dtype == torch.bool:
            raise ValueError(f"groups must be an integer device tensor of shape ({n},)")
        lo, hi = (int(groups.min()), int(groups.max())) if n else (0, 0)
        G = int(n_groups) if n_groups is not None else (out.n_groups if out is not None else hi + 1)
        if not 1 <= G <= _lib.STATS_MAXG:
            raise ValueError(f"n_groups must be 1..{_lib.STATS_MAXG}, got {G}")
        if lo < 0 or hi >= G:
            raise ValueError(f"groups must lie in [0, {G}); found [{lo}, {hi}]")
        g8 = groups.to(torch.uint8).contiguous()
    else:
        G = int(n_groups) if n_groups is not None else (out.n_groups if out is not None else 1)
        if not 1 <= G <= _lib.STATS_MAXG:
            raise ValueError(f"n_groups must be 1..{_lib.STATS_MAXG}, got {G}")
    if q is None:
        q = out.q if out is not None else fixed_q(X.abs().amax(0).double().cpu().numpy() if n else [0.0] * d)
    qa = np.ascontiguousarray(np.asarray(q, dtype=np.int32))
    if qa.shape != (d,):
        raise ValueError(f"q must hold {d} exponents")
    W = _lib.stats_words(d)
    if out is None:
        buf = torch.zeros(G * k * W + 1, dtype=torch.int64, device=X.device)
        out = ClusterStats(buf[:-1].view(G, k, W), qa.tolist(), d, _buf=buf)
    else:
        if not isinstance(out, ClusterStats) or out._buf is None or out._buf.device != X.device:
            raise ValueError("out must be a ClusterStats that cluster_stats returned on this device")
        if (out.n_groups, out.n_clusters, out.d, out.q) != (G, k, d, qa.tolist()):
            raise ValueError("out differs in (n_groups, n_clusters, d, q)")
    accumulate(X, labels, g8, G, k, qa, out._buf)
    skipped = int(out._buf[-1])
    if skipped:
        raise ValueError(f"cluster_stats skipped {skipped} rows (label or group out of range, NaN or Inf)")
    return out


@dataclass
class SurfaceElements:
    normal: np.ndarray       # (K, 3) unit eigenvector of the smallest eigenvalue, component 0 (z) >= 0
    roughness: np.ndarray    # sqrt(max(l_min, 0)): the spread along the normal
    planarity: np.ndarray    # (l_mid - l_min) / l_max, 0 where l_max == 0
    rms: np.ndarray          # sqrt(trace): the rms distance of the points to their mean
    count: np.ndarray        # (K,) int64, groups merged


def surface_elements(stats: ClusterStats, min_count: int = 3) -> SurfaceElements:
    """Per-cluster surface element of a D = 3 cloud from the covariance of the
    cluster's points (groups merged), ``np.linalg.eigh`` per cluster on the host.
    Rows are NaN where the count is below ``min_count``."""
    if stats.d != 3:
        raise ValueError("surface_elements needs d = 3")
    m = stats.merged()
    count = m.counts()[0]
    cov = m.covariances()[0]
    K = count.shape[0]
    normal = np.full((K, 3), np.nan)
    rough, plan, rms = np.full(K, np.nan), np.full(K, np.nan), np.full(K, np.nan)
    for j in np.flatnonzero(count >= max(1, int(min_count))):
        lam, vec = np.linalg.eigh(cov[j])          # ascending eigenvalues
        v = vec[:, 0]
        if v[0] < 0 or (v[0] == 0 and (v[1] < 0 or (v[1] == 0 and v[2] < 0))):
            v = -v
        normal[j] = v
        rough[j] = np.sqrt(max(lam[0], 0.0))
        plan[j] = (lam[1] - lam[0]) / lam[2] if lam[2] > 0 else 0.0
        rms[j] = np.sqrt(max(cov[j, 0, 0] + cov[j, 1, 1] + cov[j, 2, 2], 0.0))
    return SurfaceElements(normal=normal, roughness=rough, planarity=plan, rms=rms, count=count)
