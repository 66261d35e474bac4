"""Exact height-map raster of a (labelled, multi-day) cloud.

``height_grid`` runs ``pcm_height_grid`` once over ``(X[, labels][, groups])``:
for every (group, pixel) the count, the fixed-point sum of the heights, and the
highest and the lowest height each with the label of the row that holds it, as
four 64-bit integer words (DESIGN.md §4 "Height grid").  Integer adds and
maxima commute, so the words are the same bits for any row order and any split
of the rows over calls, clouds and ranks (``out=``, ``+``, ``merged``).  There
is no CPU fallback for the pass itself; the accessors work on any words
(device tensor or NumPy array).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from .fixed import QBITS, fixed_q

_BIAS = 1 << QBITS
_LOW = 0xFFFFFFFF


class HeightGrid:
    """The words of ``pcm_height_grid`` for G groups on an H x W raster.

    ``words``: int64 (G, 4, H, W) -- a device tensor as ``height_grid`` returns
    it, or a NumPy array (int64 / uint64 bit patterns); ``q``: the fixed-point
    exponent of z; ``cell_log2``: cells are 2^cell_log2 units on a side;
    ``origin``: (oy, ox); ``outside``: valid rows that fell outside the raster.
    """

    def __init__(self, words, q: int, cell_log2: int = 0, origin=(0.0, 0.0), outside: int = 0, _buf=None):
        if not isinstance(words, torch.Tensor):
            words = np.ascontiguousarray(words).view(np.int64) if np.asarray(words).dtype == np.uint64 \
                else np.ascontiguousarray(words, dtype=np.int64)
        if words.ndim != 4 or words.shape[1] != _lib.GRID_WORDS:
            raise ValueError(f"words must be (G, {_lib.GRID_WORDS}, H, W)")
        self.words = words
        self.q = int(q)
        self.cell_log2 = int(cell_log2)
        self.origin = (float(np.float32(origin[0])), float(np.float32(origin[1])))
        self.outside = int(outside)
        self._buf = _buf     # device: the (G*4*H*W + 2) buffer `words` views; then [outside, skipped]

    # ------------------------------------------------------------ shape
    @property
    def n_groups(self) -> int:
        return int(self.words.shape[0])

    @property
    def shape(self):
        return int(self.words.shape[2]), int(self.words.shape[3])

    def numpy(self) -> np.ndarray:
        """The words on the host, int64 (G, 4, H, W)."""
        w = self.words
        return w.cpu().numpy() if isinstance(w, torch.Tensor) else w

    def _same(self, other: "HeightGrid"):
        if not isinstance(other, HeightGrid) or tuple(other.words.shape) != tuple(self.words.shape) or \
                (other.q, other.cell_log2, other.origin) != (self.q, self.cell_log2, self.origin):
            raise ValueError("HeightGrids differ in shape, q, cell_log2 or origin")

    # ------------------------------------------------------------ exact
    def counts(self) -> np.ndarray:
        """int64 (G, H, W)."""
        return self.numpy()[:, 0].copy()

    def sums(self) -> np.ndarray:
        """sum zq, int64 (G, H, W)."""
        return self.numpy()[:, 1].copy()

    def _height(self, w: np.ndarray, sign: int) -> np.ndarray:
        zq = sign * ((w >> 32) - _BIAS)
        return np.where(w != 0, np.ldexp(zq.astype(np.float64), -self.q), np.nan)

    @staticmethod
    def _label(w: np.ndarray) -> np.ndarray:
        return np.where(w != 0, _LOW - (w & _LOW), -1).astype(np.int32)

    def top(self) -> np.ndarray:
        """The highest height ldexp(zq, -q) of each (group, pixel), float64, NaN where empty."""
        return self._height(self.numpy()[:, 2], 1)

    def bottom(self) -> np.ndarray:
        """The lowest height of each (group, pixel), float64, NaN where empty."""
        return self._height(self.numpy()[:, 3], -1)

    def top_labels(self) -> np.ndarray:
        """The label of the highest row (the smallest among equal heights), int32, -1 where empty."""
        return self._label(self.numpy()[:, 2])

    def bottom_labels(self) -> np.ndarray:
        return self._label(self.numpy()[:, 3])

    def merged(self) -> "HeightGrid":
        """The groups joined, as a one-group HeightGrid: words 0-1 add, words 2-3 take the maximum."""
        w = self.words
        if isinstance(w, torch.Tensor):
            m = torch.cat([w[:, :2].sum(0, keepdim=True), w[:, 2:].amax(0, keepdim=True)], dim=1)
        else:
            u = w.view(np.uint64)
            with np.errstate(over="ignore"):
                m = np.concatenate([u[:, :2].sum(0, keepdims=True, dtype=np.uint64), u[:, 2:].max(0, keepdims=True)], axis=1)
        return HeightGrid(m, self.q, self.cell_log2, self.origin, self.outside)

    def __add__(self, other: "HeightGrid") -> "HeightGrid":
        self._same(other)
        a, b = self.words, other.words
        if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
            b = b.to(a.device)
            m = torch.cat([a[:, :2] + b[:, :2], torch.maximum(a[:, 2:], b[:, 2:])], dim=1)   # words 2-3 are below 2^63
        else:
            a, b = self.numpy().view(np.uint64), other.numpy().view(np.uint64)
            with np.errstate(over="ignore"):
                m = np.concatenate([a[:, :2] + b[:, :2], np.maximum(a[:, 2:], b[:, 2:])], axis=1)
        return HeightGrid(m, self.q, self.cell_log2, self.origin, self.outside + other.outside)

    # ------------------------------------------------------------ derived (float64)
    def means(self) -> np.ndarray:
        """ldexp(float64(S), -q) / count, (G, H, W), NaN where empty."""
        n = self.counts().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.ldexp(self.sums().astype(np.float64), -self.q) / n
        m[n == 0] = np.nan
        return m

    def relief(self) -> np.ndarray:
        """top - bottom, NaN where empty."""
        return self.top() - self.bottom()


def accumulate(X: torch.Tensor, labels: Optional[torch.Tensor], k: int, groups8: Optional[torch.Tensor], n_groups: int,
               shape, origin, cell_log2: int, q: int, buf: torch.Tensor) -> None:
    """``pcm_height_grid`` on checked arguments: adds the rows' words into ``buf`` (device int64,
    n_groups * 4 * H * W + 2), stream-ordered, without any synchronisation."""
    from .engine import _ptr, _stream
    n = X.shape[0]
    rc = _lib.load().pcm_height_grid(_ptr(X) if n else None, n, _ptr(labels) if (labels is not None and n) else None, k,
                                     _ptr(groups8) if (groups8 is not None and n) else None, n_groups,
                                     int(shape[0]), int(shape[1]), ctypes.c_float(origin[0]), ctypes.c_float(origin[1]),
                                     int(cell_log2), int(q), _ptr(buf), _stream())
    _lib.check(rc, "pcm_height_grid")


def height_grid(X: torch.Tensor, shape, *, origin=(0, 0), cell_log2: int = 0, labels: Optional[torch.Tensor] = None,
                n_clusters: Optional[int] = None, groups: Optional[torch.Tensor] = None, n_groups: Optional[int] = None,
                q: Optional[int] = None, out: Optional[HeightGrid] = None) -> HeightGrid:
    """Raster the rows (z, y, x) of ``X`` (n, 3), float32, on the device, onto
    ``shape`` = (H, W) cells of 2^cell_log2 units from ``origin`` = (oy, ox).

    ``labels``: device int32 (n,) in [0, n_clusters) (default: label 0;
    ``n_clusters`` defaults to ``max + 1``).  ``groups``: any integer device
    tensor (n,) with values in [0, n_groups) -- the day or cloud of each row
    (default: one group); ``n_groups`` (<= 256) defaults to ``max + 1``.
    ``q``: the fixed-point exponent of z, default ``fixed_q([max|z|])[0]``.
    ``out``: an earlier result of the same geometry to accumulate into (chunked
    clouds, one call per day); fewer than 2^31 rows in all may go into one
    result.  Raises ValueError when rows were skipped (label or group out of
    range, NaN or Inf, |z| too large for ``q``); rows outside the raster are
    counted in ``.outside``.
    """
    if not (isinstance(X, torch.Tensor) and X.is_cuda):
        raise _lib.PcmError("height_grid expects a HIP device tensor (no CPU fallback)")
    if X.dim() != 2 or X.shape[1] != 3:
        raise ValueError("X must be (n, 3) rows of z, y, x")
    if X.dtype != torch.float32:
        raise ValueError("points dtype must be float32")
    X = X.contiguous()
    n = X.shape[0]
    H, W = int(shape[0]), int(shape[1])
    s = int(cell_log2)
    if not (1 <= H <= 1 << 24 and 1 <= W <= 1 << 24):
        raise ValueError("shape must be (H, W) with 1 <= H, W <= 2^24")
    if not -8 <= s <= 16:
        raise ValueError("cell_log2 must be -8..16")
    origin = (float(np.float32(origin[0])), float(np.float32(origin[1])))
    k = 1
    if labels is not None:
        if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int32 and
                tuple(labels.shape) == (n,)):
            raise ValueError(f"labels must be a device int32 tensor of shape ({n},)")
        labels = labels.contiguous()
        k = int(n_clusters) if n_clusters is not None else (int(labels.max()) + 1 if n else 1)
        if k < 1:
            raise ValueError("n_clusters must be >= 1")
    g8 = None
    if groups is not None:
        if not (isinstance(groups, torch.Tensor) and groups.is_cuda and tuple(groups.shape) == (n,)) or \
                groups.dtype.is_floating_point or groups.dtype == torch.bool:
            raise ValueError(f"groups must be an integer device tensor of shape ({n},)")
        lo, hi = (int(groups.min()), int(groups.max())) if n else (0, 0)
        G = int(n_groups) if n_groups is not None else (out.n_groups if out is not None else hi + 1)
        if not 1 <= G <= _lib.GRID_MAXG:
            raise ValueError(f"n_groups must be 1..{_lib.GRID_MAXG}, got {G}")
        if lo < 0 or hi >= G:
            raise ValueError(f"groups must lie in [0, {G}); found [{lo}, {hi}]")
        g8 = groups.to(torch.uint8).contiguous()
    else:
        G = int(n_groups) if n_groups is not None else (out.n_groups if out is not None else 1)
        if not 1 <= G <= _lib.GRID_MAXG:
            raise ValueError(f"n_groups must be 1..{_lib.GRID_MAXG}, got {G}")
    if G * H * W >= 1 << 31:
        raise ValueError("n_groups * H * W must be below 2^31")
    if q is None:
        q = out.q if out is not None else fixed_q([float(X[:, 0].abs().max()) if n else 0.0])[0]
    q = int(q)
    if out is None:
        buf = torch.zeros(G * _lib.GRID_WORDS * H * W + 2, dtype=torch.int64, device=X.device)
        out = HeightGrid(buf[:-2].view(G, _lib.GRID_WORDS, H, W), q, s, origin, 0, _buf=buf)
    else:
        if not isinstance(out, HeightGrid) or out._buf is None or out._buf.device != X.device:
            raise ValueError("out must be a HeightGrid that height_grid returned on this device")
        if (out.n_groups, out.shape, out.q, out.cell_log2, out.origin) != (G, (H, W), q, s, origin):
            raise ValueError("out differs in (n_groups, shape, q, cell_log2, origin)")
    accumulate(X, labels, k, g8, G, (H, W), origin, s, q, out._buf)
    outside, skipped = (int(v) for v in out._buf[-2:].tolist())
    out.outside = outside
    if skipped:
        raise ValueError(f"height_grid skipped {skipped} rows (label or group out of range, NaN or Inf, "
                         f"or |z| >= 2^{QBITS - q})")
    return out
