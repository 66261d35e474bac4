"""Exact voxel-grid reduction of a cloud, and the thinning built on it.

``voxel_grid`` gives one entry per occupied voxel of a lattice anchored at ``origin`` -- not at the
cloud, so the voxels of two clouds or two days are the same voxels: the count, the exact
fixed-point coordinate sums (hence the exact centroid), the lowest row and, with ``groups``, the
days that saw the voxel (DESIGN.md §4 "Voxels").  ``pcm_voxel_keys`` gives every row the key of its
cell, ``torch.sort`` orders the keys (plumbing; nothing depends on its stability),
``pcm_voxel_count`` counts the voxels, one host read sizes the outputs and ``pcm_voxel_reduce``
fills them.  Every output is an integer: one answer for any row order.  ``voxel_downsample`` keeps
one point per voxel.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .fixed import fixed_q
from .support import _check_points, _groups8

MAXG = _lib.VOXEL_MAXG


def voxel_sizes(voxel) -> Tuple[np.ndarray, np.ndarray]:
    """A scalar or (vz, vy, vx) -> (float32 sizes (3,), float32 inverses (3,)), checked."""
    try:
        with np.errstate(over="ignore"):
            v = np.asarray(voxel, dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"voxel must be a number or three numbers (vz, vy, vx), got {voxel!r}") from None
    if v.shape == ():
        v = np.full(3, v, dtype=np.float32)
    if v.shape != (3,):
        raise ValueError(f"voxel must be a number or three numbers (vz, vy, vx), got {voxel!r}")
    if not (np.isfinite(v).all() and (v > 0).all()):
        raise ValueError(f"voxel sizes must be finite and > 0 in float32, got {voxel!r}")
    with np.errstate(over="ignore"):
        inv = (1.0 / v.astype(np.float64)).astype(np.float32)
    if not (np.isfinite(inv).all() and (inv >= np.finfo(np.float32).tiny).all()):
        raise ValueError(f"voxel sizes must have a finite, normal float32 inverse, got {voxel!r}")
    return v, inv


def _origin32(origin) -> np.ndarray:
    try:
        with np.errstate(over="ignore"):
            o = np.asarray(origin, dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"origin must be three numbers (oz, oy, ox), got {origin!r}") from None
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError(f"origin must be three finite float32 numbers (oz, oy, ox), got {origin!r}")
    return o


def _decode_box(words) -> np.ndarray:
    """info[9..14], the order-preserving uint32 of the box -> float32 (6,), low corner then high."""
    u = np.asarray(words, dtype=np.int64).astype(np.uint32)
    bits = np.where(u >> 31, u & np.uint32(0x7fffffff), ~u)
    return bits.astype(np.uint32).view(np.float32)


def _popcount64(mask: torch.Tensor) -> torch.Tensor:
    def pop32(v):   # v: int64 holding a value below 2^32
        v = v - ((v >> 1) & 0x55555555)
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
        v = (v + (v >> 4)) & 0x0f0f0f0f
        return ((v * 0x01010101) >> 24) & 0xff
    return (pop32(mask & 0xffffffff) + pop32((mask >> 32) & 0xffffffff)).to(torch.int32)


@dataclass
class Voxels:
    cells: torch.Tensor                 # device int64 (M, 3): absolute cell indices (cz, cy, cx), ascending
    counts: torch.Tensor                # device int32 (M,): rows in the voxel
    sums: torch.Tensor                  # device int64 (M, 3): exact sums of trunc(ldexp(x_a, q_a))
    first: torch.Tensor                 # device int32 (M,): the lowest row index in the voxel
    day_mask: Optional[torch.Tensor]    # device int64 (M,): bit g set iff a row of group g is in the voxel; None without groups
    inverse: torch.Tensor               # device int32 (n,): the voxel of every row, -1 for a non-finite row
    skipped: int                        # rows with a NaN or Inf coordinate
    voxel: Tuple[float, float, float]   # the float32 sizes (vz, vy, vx)
    inv: Tuple[float, float, float]     # the float32 factors the cells were formed with
    origin: Tuple[float, float, float]
    q: list                             # the fixed-point exponents of ``sums``

    def centroids(self) -> torch.Tensor:
        """float32 of (float64(S) * 2^-q) / float64(count): ``ClusterStats.means()``'s formula; device (M, 3)."""
        scale = torch.tensor(np.ldexp(1.0, -np.asarray(self.q, dtype=np.int64)), dtype=torch.float64,
                             device=self.sums.device)
        return ((self.sums.to(torch.float64) * scale) / self.counts.to(torch.float64)[:, None]).to(torch.float32)

    def days(self) -> torch.Tensor:
        """The number of groups that saw each voxel: device int32 (M,)."""
        if self.day_mask is None:
            raise ValueError("days() needs a voxel_grid call with groups")
        return _popcount64(self.day_mask)


def workspace(n: int, device) -> torch.Tensor:
    nbytes = ctypes.c_size_t()
    _lib.check(_lib.load().pcm_voxel_workspace(int(n), ctypes.byref(nbytes)), "pcm_voxel_workspace")
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def voxel_keys(X: torch.Tensor, v32: np.ndarray, o32: np.ndarray):
    """``pcm_voxel_keys`` on checked arguments -> (keys int64 (n,), info int64 (16,)), both on the device."""
    from .engine import _ptr, _stream
    n = int(X.shape[0])
    keys = torch.empty(n, dtype=torch.int64, device=X.device)
    info = torch.empty(_lib.VOXEL_INFO_WORDS, dtype=torch.int64, device=X.device)
    rc = _lib.load().pcm_voxel_keys(_ptr(X) if n else None, n, v32.ctypes.data_as(ctypes.c_void_p),
                                    o32.ctypes.data_as(ctypes.c_void_p), _ptr(keys) if n else None, _ptr(info), _stream())
    _lib.check(rc, "pcm_voxel_keys")
    return keys, info


def voxel_count(sorted_keys: torch.Tensor, info: torch.Tensor, ws: torch.Tensor) -> None:
    """``pcm_voxel_count``: the number of voxels into ``info[8]``; stream-ordered, no synchronisation."""
    from .engine import _ptr, _stream
    rc = _lib.load().pcm_voxel_count(_ptr(sorted_keys), int(sorted_keys.numel()), _ptr(info), _ptr(ws), int(ws.numel()),
                                     _stream())
    _lib.check(rc, "pcm_voxel_count")


def voxel_reduce(X: torch.Tensor, groups8: Optional[torch.Tensor], n_groups: int, qa: np.ndarray,
                 sorted_keys: torch.Tensor, perm: torch.Tensor, m: int, info: torch.Tensor, ws: torch.Tensor):
    """``pcm_voxel_reduce`` on checked arguments -> (cells, counts, sums, first, day_mask or None, inverse)."""
    from .engine import _ptr, _stream
    n, dev = int(X.shape[0]), X.device
    cells = torch.empty((m, 3), dtype=torch.int64, device=dev)
    counts = torch.empty(m, dtype=torch.int32, device=dev)
    sums = torch.empty((m, 3), dtype=torch.int64, device=dev)
    first = torch.empty(m, dtype=torch.int32, device=dev)
    mask = torch.empty(m, dtype=torch.int64, device=dev) if groups8 is not None else None
    inverse = torch.empty(n, dtype=torch.int32, device=dev)
    opt = lambda t: _ptr(t) if (t is not None and t.numel()) else None   # noqa: E731
    rc = _lib.load().pcm_voxel_reduce(_ptr(X), n, _ptr(groups8) if groups8 is not None else None, n_groups,
                                      qa.ctypes.data_as(ctypes.c_void_p), _ptr(sorted_keys), _ptr(perm), m, opt(cells),
                                      opt(counts), opt(sums), opt(first), opt(mask), _ptr(inverse), _ptr(info), _ptr(ws),
                                      int(ws.numel()), _stream())
    _lib.check(rc, "pcm_voxel_reduce")
    return cells, counts, sums, first, mask, inverse


def _raise_for(err: int, voxel) -> None:
    if err & _lib.VOXEL_E_NONFINITE:
        raise ValueError(f"voxel={voxel!r}: a cell index of the cloud's bounding box is not finite in float32")
    if err & _lib.VOXEL_E_MAGNITUDE:
        raise ValueError(f"voxel={voxel!r} is too fine for this cloud: a cell index exceeds 2^40 in magnitude")
    if err:
        raise ValueError(f"voxel={voxel!r} is too fine for this cloud: an axis spans more than 2^21 cells")


def voxel_grid(X: torch.Tensor, voxel, *, origin=(0.0, 0.0, 0.0), groups: Optional[torch.Tensor] = None,
               n_groups: Optional[int] = None, q=None) -> Voxels:
    """Reduce the rows (z, y, x) of ``X`` (n, 3), float32, on the device, to the occupied voxels of a lattice.

    ``voxel``: one size or ``(vz, vy, vx)``, positive finite float32.  On axis a the cell of a finite
    row is ``floorf((x_a - origin_a) * inv_a)`` in float32, ``inv_a = float32(1 / float64(v_a))``:
    power-of-two sizes give exact boundaries, for other sizes this rule is the definition and
    ``Voxels.inv`` reports the factor.  A row with a NaN or Inf coordinate belongs to no voxel: it is
    counted in ``skipped`` and gets ``inverse = -1``.  The M voxels come in ascending (cz, cy, cx)
    order whatever the row order.  ``groups``: any integer device tensor (n,) with values in
    [0, n_groups), ``n_groups`` <= 64 (default ``max + 1``).  ``q``: the three fixed-point exponents
    of ``sums``, default ``fixed_q`` of max|x| over the finite rows.

    Raises ValueError naming ``voxel`` when, over the finite rows' bounding box, a cell index is not
    finite, exceeds 2^40 in magnitude, or an axis spans more than 2^21 cells (all three spanning
    exactly 2^21 included): there is no silent coarsening.
    """
    X = _check_points(X, "voxel_grid")
    n = int(X.shape[0])
    v32, inv = voxel_sizes(voxel)
    o32 = _origin32(origin)
    g8, G = _groups8(groups, n, n_groups)
    qa = None
    if q is not None:
        qa = np.ascontiguousarray(np.asarray(q, dtype=np.int32))
        if qa.shape != (3,):
            raise ValueError("q must hold 3 exponents")
    keys, info = voxel_keys(X, v32, o32)
    skeys = perm = ws = None
    if n:
        skeys, perm = torch.sort(keys)
        ws = workspace(n, X.device)
        voxel_count(skeys, info, ws)
    host = info.tolist()                       # the one host read: error word, M, skipped, the box
    _raise_for(int(host[0]), voxel)
    m = int(host[8])
    if qa is None:
        box = _decode_box(host[9:15]) if m else np.zeros(6, dtype=np.float32)
        qa = np.asarray(fixed_q(np.maximum(np.abs(box[:3]), np.abs(box[3:])).astype(np.float64)), dtype=np.int32)
    if n:
        cells, counts, sums, first, mask, inverse = voxel_reduce(X, g8, G, qa, skeys, perm, m, info, ws)
        if int(info[15]):
            raise _lib.PcmError("voxel_grid: the sort did not return a permutation")
    else:
        dev = X.device
        cells, sums = (torch.empty((0, 3), dtype=torch.int64, device=dev) for _ in range(2))
        counts, first, inverse = (torch.empty(0, dtype=torch.int32, device=dev) for _ in range(3))
        mask = torch.empty(0, dtype=torch.int64, device=dev) if g8 is not None else None
    return Voxels(cells=cells, counts=counts, sums=sums, first=first, day_mask=mask, inverse=inverse,
                  skipped=int(host[7]), voxel=tuple(float(x) for x in v32), inv=tuple(float(x) for x in inv),
                  origin=tuple(float(x) for x in o32), q=[int(x) for x in qa])


@dataclass
class Downsampled:
    points: torch.Tensor    # device float32 (M', 3): one point per kept voxel, in voxel order
    rows: torch.Tensor      # device int32 (M',): the ``first`` row of each kept voxel: per-row properties can follow
    kept: torch.Tensor      # device bool (M,): which voxels of ``voxels`` were kept
    voxels: Voxels


def _downsample_args(mode, min_count, min_days, groups) -> None:
    if mode not in ("centroid", "first"):
        raise ValueError(f"mode must be 'centroid' or 'first', got {mode!r}")
    if int(min_count) != min_count or min_count < 1:
        raise ValueError(f"min_count must be an integer >= 1, got {min_count!r}")
    if int(min_days) != min_days or min_days < 1:
        raise ValueError(f"min_days must be an integer >= 1, got {min_days!r}")
    if min_days > 1 and groups is None:
        raise ValueError("min_days > 1 needs groups")


def voxel_downsample(X: torch.Tensor, voxel, *, mode: str = "centroid", origin=(0.0, 0.0, 0.0), min_count: int = 1,
                     min_days: int = 1, groups: Optional[torch.Tensor] = None,
                     n_groups: Optional[int] = None) -> Downsampled:
    """The voxel-grid filter: one point per occupied voxel of ``voxel_grid(X, voxel, origin=...)``.

    ``mode="centroid"``: the exact centroid of the voxel's rows (``Voxels.centroids()``);
    ``mode="first"``: ``X[first]``, a measured point.  Voxels with fewer than ``min_count`` rows or
    (``groups`` given) seen by fewer than ``min_days`` groups are dropped: the multi-day
    persistence filter.  ``min_days`` > 1 needs groups.
    """
    _downsample_args(mode, min_count, min_days, groups)
    X = _check_points(X, "voxel_downsample")
    vox = voxel_grid(X, voxel, origin=origin, groups=groups, n_groups=n_groups)
    kept = vox.counts >= int(min_count)
    if min_days > 1:
        kept &= vox.days() >= int(min_days)
    rows = vox.first[kept]
    points = vox.centroids()[kept] if mode == "centroid" else X[rows.long()]
    return Downsampled(points=points.contiguous(), rows=rows, kept=kept, voxels=vox)
