"""Exact nearest row of another cloud within a radius: the cloud-to-cloud distance.

``kmeans_assign``'s ``residual`` is the distance to a centre that stands for thousands of
points: it measures the size of a surface element, not change.  ``nearest_points`` gives, for
every row of a later cloud, the nearest row of an earlier one within ``max_dist``, its squared
distance and -- through the index -- its height (DESIGN.md §4 "Nearest"): ``pcm_nearest_keys``
gives the rows of both clouds the keys of their cells in one common box, ``torch.sort`` orders
the two key arrays (plumbing), ``pcm_nearest_find`` gathers the cell-sorted copy of the targets
and scans the 27 cells around each query.  The distance is the canonical float32 direct form and
a tie goes to the lowest target row, so index and distance are one answer for any row order.
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib

I_SKIPPED, I_SKIPPED_TARGETS, I_BADPERM = 7, 8, 16     # words of the info block (include/pcm_kmeans.h)


@dataclass
class Nearest:
    index: torch.Tensor       # device int32 (n,): the nearest target row within max_dist, -1 when there is none
    sqdist: torch.Tensor      # device float32 (n,): its squared distance, +inf when there is none
    skipped: int              # query rows with a NaN or Inf coordinate (-1 / +inf)
    skipped_targets: int      # target rows with a NaN or Inf coordinate (never returned)
    max_dist: float           # the float32 radius the kernel compared with
    cell_log2: int            # the cells were 2^cell_log2 units on a side

    def found(self) -> torch.Tensor:
        """Device bool (n,): the rows that have a candidate."""
        return self.index >= 0

    def distance(self) -> torch.Tensor:
        """Device float32 (n,): ``sqrt(sqdist)``, +inf when there is none."""
        return torch.sqrt(self.sqdist)


def _max_dist32(max_dist) -> np.float32:
    try:
        with np.errstate(over="ignore", under="ignore"):
            r = np.float32(max_dist)
            r2 = np.float32(r * r)
    except (TypeError, ValueError):
        raise ValueError(f"max_dist must be a number, got {max_dist!r}") from None
    if not (np.isfinite(r) and r > 0):
        raise ValueError(f"max_dist must be finite and > 0 in float32, got {max_dist!r}")
    if not (np.isfinite(r2) and r2 > 0):
        raise ValueError(f"max_dist squared must be finite and > 0 in float32 (+inf means 'none'), got {max_dist!r}")
    return r


def _check_points(X, name: str) -> torch.Tensor:
    if not (isinstance(X, torch.Tensor) and X.is_cuda):
        raise _lib.PcmError(f"nearest_points expects HIP device tensors (no CPU fallback): {name} is not one")
    if X.dim() != 2 or X.shape[1] != 3 or X.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 (n, 3) tensor in z, y, x order")
    if X.shape[0] >= 1 << 31:
        raise ValueError(f"{name} must hold fewer than 2^31 rows")
    return X.contiguous()


def _groups32(groups, rows: int, name: str) -> torch.Tensor:
    if not (isinstance(groups, torch.Tensor) and groups.is_cuda and tuple(groups.shape) == (rows,)) or \
            groups.dtype.is_floating_point or groups.dtype == torch.bool or groups.dtype.is_complex:
        raise ValueError(f"{name} must be an integer device tensor of shape ({rows},)")
    if groups.dtype == torch.int32:
        return groups.contiguous()
    if groups.dtype not in (torch.int8, torch.uint8, torch.int16) and rows:     # a dtype wider than int32
        lo, hi = int(groups.min()), int(groups.max())
        if lo < -(1 << 31) or hi >= 1 << 31:
            raise ValueError(f"{name} must hold int32 values; found [{lo}, {hi}]")
    return groups.to(torch.int32).contiguous()


def nearest_keys(X: torch.Tensor, Y: torch.Tensor, r: np.float32):
    """``pcm_nearest_keys`` on checked arguments -> (xkeys int64 (n,), ykeys int64 (m,), info int64 (20,)), on the device."""
    from .engine import _ptr, _stream
    n, m = int(X.shape[0]), int(Y.shape[0])
    xkeys = torch.empty(n, dtype=torch.int64, device=X.device)
    ykeys = torch.empty(m, dtype=torch.int64, device=X.device)
    info = torch.empty(_lib.NEAREST_INFO_WORDS, dtype=torch.int64, device=X.device)
    rc = _lib.load().pcm_nearest_keys(_ptr(X) if n else None, n, _ptr(Y) if m else None, m, ctypes.c_float(float(r)),
                                      _ptr(xkeys) if n else None, _ptr(ykeys) if m else None, _ptr(info), _stream())
    _lib.check(rc, "pcm_nearest_keys")
    return xkeys, ykeys, info


def workspace(m: int, device) -> torch.Tensor:
    nbytes = ctypes.c_size_t()
    _lib.check(_lib.load().pcm_nearest_workspace(int(m), ctypes.byref(nbytes)), "pcm_nearest_workspace")
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def nearest_find(X: torch.Tensor, Y: torch.Tensor, g32: Optional[torch.Tensor], tg32: Optional[torch.Tensor],
                 r: np.float32, xskeys: Optional[torch.Tensor], xperm: Optional[torch.Tensor],
                 yskeys: Optional[torch.Tensor], yperm: Optional[torch.Tensor], info: torch.Tensor,
                 ws: Optional[torch.Tensor], index: torch.Tensor, sqdist: torch.Tensor) -> None:
    """``pcm_nearest_find`` on checked arguments: stream-ordered, no synchronisation."""
    from .engine import _ptr, _stream

    def ptr(t):
        return _ptr(t) if t is not None and t.numel() else None

    rc = _lib.load().pcm_nearest_find(ptr(X), int(X.shape[0]), ptr(Y), int(Y.shape[0]), ptr(g32), ptr(tg32),
                                      ctypes.c_float(float(r)), ptr(xskeys), ptr(xperm), ptr(yskeys), ptr(yperm),
                                      ptr(index), ptr(sqdist), _ptr(info), ptr(ws), int(ws.numel()) if ws is not None else 0,
                                      _stream())
    _lib.check(rc, "pcm_nearest_find")


def nearest_points(X: torch.Tensor, Y: torch.Tensor, max_dist: float, *, groups: Optional[torch.Tensor] = None,
                   target_groups: Optional[torch.Tensor] = None) -> Nearest:
    """For every row (z, y, x) of ``X`` (n, 3) the nearest row of ``Y`` (m, 3) within ``max_dist``; float32, on the device.

    Target j is a candidate of query i iff both rows are finite and ``d2 = (dz*dz + dy*dy) + dx*dx
    <= r*r`` in float32 (r = float32(max_dist), differences X[i] - Y[j], no FMA) and -- with
    ``groups`` (n,) and ``target_groups`` (m,), integer device tensors of any int32 values, given
    together -- ``groups[i] != target_groups[j]``.  ``index[i]`` is the candidate with the smallest
    ``(d2, j)``: a tie in distance goes to the LOWEST target row; -1 when there is none.
    ``sqdist[i]`` is that ``d2``, +inf when there is none.  ``X`` and ``Y`` may be one tensor:
    ``groups=target_groups=arange(n)`` then excludes a row itself, day labels give the nearest point
    of another day.  A query with a NaN or Inf coordinate gets -1 / +inf (``skipped``); such a
    target is never returned (``skipped_targets``).  ``max_dist`` is required -- the cells prune by
    it -- and its float32 square must be finite, so that +inf can mean "none".

    The scan tests a query against every target of the cells around it: its cost grows with the
    product of the cells' populations (DESIGN.md §4 "Nearest").
    """
    X = _check_points(X, "X")
    Y = _check_points(Y, "Y")
    if Y.device != X.device:
        raise ValueError("X and Y must be on the same device")
    n, m = int(X.shape[0]), int(Y.shape[0])
    r = _max_dist32(max_dist)
    if (groups is None) != (target_groups is None):
        raise ValueError("groups and target_groups go together: give both or neither")
    g32 = tg32 = None
    if groups is not None:
        g32, tg32 = _groups32(groups, n, "groups"), _groups32(target_groups, m, "target_groups")
    index = torch.empty(n, dtype=torch.int32, device=X.device)
    sqdist = torch.empty(n, dtype=torch.float32, device=X.device)
    xkeys, ykeys, info = nearest_keys(X, Y, r)
    if n and m:
        xskeys, xperm = torch.sort(xkeys)
        yskeys, yperm = torch.sort(ykeys)
        nearest_find(X, Y, g32, tg32, r, xskeys, xperm, yskeys, yperm, info, workspace(m, X.device), index, sqdist)
    elif n:
        nearest_find(X, Y, None, None, r, None, None, None, None, info, None, index, sqdist)
    host = info.tolist()
    if host[I_BADPERM]:
        raise _lib.PcmError("nearest_points: a sort did not return a permutation")
    return Nearest(index=index, sqdist=sqdist, skipped=int(host[I_SKIPPED]), skipped_targets=int(host[I_SKIPPED_TARGETS]),
                   max_dist=float(r), cell_log2=int(host[0]))
