"""Exact neighbour and day-support counts of a cloud, and the radius outlier filter built on them.

SGBM/WLS disparity leaves speckle: isolated points far above or below the
surface, seen by one pair on one day.  ``radius_support`` counts, for every row,
the other rows within ``radius`` of it and -- with ``groups`` -- the distinct days
among the row and those neighbours (DESIGN.md §4 "Support"): ``pcm_support_keys``
gives every row the key of its cell, ``torch.sort`` orders the keys (plumbing),
``pcm_support_count`` gathers the cell-sorted copy and scans the 27 cells around
each row.  The distance is the canonical float32 direct form and the results are
integers, so they are one answer for any row order.  ``filter_outliers`` turns
them into the keep mask.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib

MAXG = _lib.SUPPORT_MAXG


@dataclass
class Support:
    counts: torch.Tensor            # device int32 (n,): neighbours within the radius, at most max_count
    days: Optional[torch.Tensor]    # device int32 (n,): distinct groups among the row and its neighbours; None without groups
    skipped: int                    # rows with a NaN or Inf coordinate (counts = days = 0)
    radius: float                   # the float32 radius the kernel compared with
    cell_log2: int                  # the cells were 2^cell_log2 units on a side


def _radius32(radius) -> np.float32:
    try:
        with np.errstate(over="ignore"):
            r = np.float32(radius)
    except (TypeError, ValueError):
        raise ValueError(f"radius must be a number, got {radius!r}") from None
    if not (np.isfinite(r) and r > 0):
        raise ValueError(f"radius must be finite and > 0 in float32, got {radius!r}")
    return r


def _check_points(X, what: str) -> torch.Tensor:
    if not (isinstance(X, torch.Tensor) and X.is_cuda):
        raise _lib.PcmError(f"{what} expects a HIP device tensor (no CPU fallback)")
    if X.dim() != 2 or X.shape[1] != 3 or X.dtype != torch.float32:
        raise ValueError("X must be a float32 (n, 3) tensor in z, y, x order")
    if X.shape[0] >= 1 << 31:
        raise ValueError("X must hold fewer than 2^31 rows")
    return X.contiguous()


def _groups8(groups, n: int, n_groups):
    if groups is None:
        if n_groups is not None and not 1 <= int(n_groups) <= MAXG:
            raise ValueError(f"n_groups must be 1..{MAXG}, got {n_groups}")
        return None, 1
    if not (isinstance(groups, torch.Tensor) and groups.is_cuda and tuple(groups.shape) == (n,)) or \
            groups.dtype.is_floating_point or groups.dtype == torch.bool:
        raise ValueError(f"groups must be an integer device tensor of shape ({n},)")
    lo, hi = (int(groups.min()), int(groups.max())) if n else (0, 0)
    G = int(n_groups) if n_groups is not None else hi + 1
    if not 1 <= G <= MAXG:
        raise ValueError(f"n_groups must be 1..{MAXG}, got {G}: days are one 64-bit mask per row")
    if lo < 0 or hi >= G:
        raise ValueError(f"groups must lie in [0, {G}); found [{lo}, {hi}]")
    return groups.to(torch.uint8).contiguous(), G


def support_keys(X: torch.Tensor, radius: np.float32):
    """``pcm_support_keys`` on checked arguments -> (keys int64 (n,), info int64 (16,)), both on the device."""
    from .engine import _ptr, _stream
    n = int(X.shape[0])
    keys = torch.empty(n, dtype=torch.int64, device=X.device)
    info = torch.empty(_lib.SUPPORT_INFO_WORDS, dtype=torch.int64, device=X.device)
    rc = _lib.load().pcm_support_keys(_ptr(X) if n else None, n, ctypes.c_float(float(radius)),
                                      _ptr(keys) if n else None, _ptr(info), _stream())
    _lib.check(rc, "pcm_support_keys")
    return keys, info


def support_count(X: torch.Tensor, groups8: Optional[torch.Tensor], n_groups: int, radius: np.float32, max_count: int,
                  sorted_keys: torch.Tensor, perm: torch.Tensor, info: torch.Tensor, ws: torch.Tensor,
                  counts: torch.Tensor, days: Optional[torch.Tensor]) -> None:
    """``pcm_support_count`` on checked arguments: stream-ordered, no synchronisation."""
    from .engine import _ptr, _stream
    n = int(X.shape[0])
    rc = _lib.load().pcm_support_count(_ptr(X), n, _ptr(groups8) if groups8 is not None else None, n_groups,
                                       ctypes.c_float(float(radius)), int(max_count), _ptr(sorted_keys), _ptr(perm),
                                       _ptr(counts), _ptr(days) if days is not None else None, _ptr(info), _ptr(ws),
                                       int(ws.numel()), _stream())
    _lib.check(rc, "pcm_support_count")


def workspace(n: int, device) -> torch.Tensor:
    nbytes = ctypes.c_size_t()
    _lib.check(_lib.load().pcm_support_workspace(int(n), ctypes.byref(nbytes)), "pcm_support_workspace")
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def radius_support(X: torch.Tensor, radius: float, *, groups: Optional[torch.Tensor] = None,
                   n_groups: Optional[int] = None, max_count: Optional[int] = None) -> Support:
    """Count, for every row (z, y, x) of ``X`` (n, 3), float32, on the device, the other rows within ``radius``.

    Row j is a neighbour of row i (j != i) iff ``(dz*dz + dy*dy) + dx*dx <= r*r`` in float32
    (r = float32(radius), differences i - j, no FMA): symmetric, duplicates count, a row is not its
    own neighbour.  ``counts`` is ``min(true count, max_count)`` (None: no limit; a limit lets the
    scan stop early when there are no groups).  ``groups``: any integer device tensor (n,) with
    values in [0, n_groups) -- the day or cloud of each row; ``n_groups`` (<= 64) defaults to
    ``max + 1``.  With groups, ``days`` is the number of distinct groups among the row and ALL its
    neighbours, whatever ``max_count`` is.  A row with a NaN or Inf coordinate has no neighbours, is
    nobody's neighbour, gets 0 and 0 and is counted in ``skipped``.

    The scan tests a row against every row of the cells around it: its cost grows with the square
    of a cell's population (DESIGN.md §4 "Support").
    """
    X = _check_points(X, "radius_support")
    n = int(X.shape[0])
    r = _radius32(radius)
    g8, G = _groups8(groups, n, n_groups)
    if max_count is None:
        maxc = -1
    else:
        maxc = int(max_count)
        if maxc < 0 or maxc >= 1 << 31 or maxc != max_count:
            raise ValueError(f"max_count must be None or an integer in [0, 2^31), got {max_count!r}")
    counts = torch.empty(n, dtype=torch.int32, device=X.device)
    days = torch.empty(n, dtype=torch.int32, device=X.device) if g8 is not None else None
    keys, info = support_keys(X, r)
    if n:
        skeys, perm = torch.sort(keys)
        support_count(X, g8, G, r, maxc, skeys, perm, info, workspace(n, X.device), counts, days)
    host = info.tolist()
    if host[15]:
        raise _lib.PcmError("radius_support: the sort did not return a permutation")
    return Support(counts=counts, days=days, skipped=int(host[7]), radius=float(r), cell_log2=int(host[0]))


def filter_outliers(X: torch.Tensor, radius: float, min_neighbors: int = 1, *, min_days: int = 1,
                    groups: Optional[torch.Tensor] = None, n_groups: Optional[int] = None) -> torch.Tensor:
    """The radius outlier filter: a device bool mask (n,), True for the rows to keep.

    A row is kept when it has at least ``min_neighbors`` other rows within ``radius`` and
    (``groups`` given) at least ``min_days`` distinct groups among itself and its neighbours; rows
    with a NaN or Inf coordinate are dropped.  One ``radius_support`` pass with
    ``max_count = min_neighbors``.
    """
    if int(min_neighbors) != min_neighbors or min_neighbors < 0:
        raise ValueError(f"min_neighbors must be an integer >= 0, got {min_neighbors!r}")
    if int(min_days) != min_days or min_days < 1:
        raise ValueError(f"min_days must be an integer >= 1, got {min_days!r}")
    if min_days > 1 and groups is None:
        raise ValueError("min_days > 1 needs groups")
    X = _check_points(X, "filter_outliers")
    sup = radius_support(X, radius, groups=groups, n_groups=n_groups, max_count=int(min_neighbors))
    keep = (sup.counts >= int(min_neighbors)) & torch.isfinite(X).all(dim=1)
    if sup.days is not None:
        keep &= sup.days >= int(min_days)
    return keep
