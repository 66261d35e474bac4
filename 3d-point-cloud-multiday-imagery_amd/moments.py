"""Exact per-point neighbourhood moments and the local surface at a point: its plane, normal and roughness.

``cluster_stats`` / ``surface_elements`` give a plane per centre, and a centre stands for
thousands of points.  ``local_moments`` gives every row the exact integer moments of the rows of
another cloud (or of its own) within ``radius`` (DESIGN.md §4 "Local moments"):
``pcm_nearest_keys`` gives the rows of both clouds the keys of their cells in one common box,
``torch.sort`` orders the key arrays (plumbing), ``pcm_moments_scan`` gathers the cell-sorted copy
of the targets and sums, over the 27 cells around each query, the fixed-point offsets of the
targets that satisfy ``nearest_points``' float32 predicate and their products.  The ten int64
words of a row are one answer for any row order.  ``point_normals`` turns them into a plane per
row (``pcm_moments_planes``, float64): the normal, the roughness, the planarity and the signed
point-to-plane distance -- with ``targets=`` an earlier day, the change along the surface normal.
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .fixed import fixed_q
from .nearest import I_BADPERM, I_SKIPPED, I_SKIPPED_TARGETS, nearest_keys

Q_MIN, Q_MAX = -126, 62      # the exponents pcm_moments_scan accepts


@dataclass
class LocalMoments:
    words: torch.Tensor       # device int64 (n, 10): count, sum dq (z, y, x), sum dq_a dq_b (zz, zy, zx, yy, yx, xx)
    q: Tuple[int, int, int]   # the fixed-point exponents: dq_a = trunc(ldexp(Y[j,a], q_a)) - trunc(ldexp(X[i,a], q_a))
    radius: float             # the float32 radius the kernel compared with
    skipped: int              # query rows with a NaN or Inf coordinate (ten zeros)
    skipped_targets: int      # target rows with a NaN or Inf coordinate (in no neighbourhood)
    cell_log2: int            # the cells were 2^cell_log2 units on a side

    def counts(self) -> torch.Tensor:
        """Device int64 (n,): the targets within the radius (the row itself included when the targets are the queries)."""
        return self.words[:, 0]

    def _scale(self, exps) -> torch.Tensor:
        return torch.tensor([math.ldexp(1.0, -int(e)) for e in exps], dtype=torch.float64, device=self.words.device)

    def offsets(self) -> torch.Tensor:
        """Device float64 (n, 3): the mean offset of the neighbourhood from the query, NaN where the count is 0."""
        c = self.words[:, 0].double()
        return self.words[:, 1:4].double() * self._scale(self.q) / c[:, None]

    def covariances(self) -> torch.Tensor:
        """Device float64 (n, 3, 3): the covariance of the neighbourhood (unbiased=False), NaN where the count is 0."""
        q = self.q
        c = self.words[:, 0].double()
        mu = self.offsets()
        second = self.words[:, 4:10].double() * self._scale([q[0] + q[0], q[0] + q[1], q[0] + q[2], q[1] + q[1], q[1] + q[2],
                                                             q[2] + q[2]]) / c[:, None]
        idx = torch.tensor([[0, 1, 2], [1, 3, 4], [2, 4, 5]], device=self.words.device)
        return second[:, idx] - mu[:, :, None] * mu[:, None, :]


@dataclass
class PointNormals:
    normal: torch.Tensor      # device float32 (n, 3): the unit normal (z, y, x) of the plane, z >= 0; NaN where not valid
    distance: torch.Tensor    # device float32 (n,): the signed distance of the row to the plane, + on the +z side
    roughness: torch.Tensor   # device float32 (n,): sqrt(max(l0, 0)), the spread along the normal
    planarity: torch.Tensor   # device float32 (n,): (l1 - l0) / l2, 0 where l2 <= 0
    count: torch.Tensor       # device int64 (n,): the targets within the radius
    min_count: int            # rows with fewer targets are NaN
    moments: LocalMoments     # the words the planes were solved from

    def valid(self) -> torch.Tensor:
        """Device bool (n,): the rows that have a plane."""
        return self.count >= max(self.min_count, 1)


def _radius32(radius) -> np.float32:
    try:
        with np.errstate(over="ignore", under="ignore"):
            r = np.float32(radius)
            r2 = np.float32(r * r)
    except (TypeError, ValueError):
        raise ValueError(f"radius must be a number, got {radius!r}") from None
    if not (np.isfinite(r) and r > 0):
        raise ValueError(f"radius must be finite and > 0 in float32, got {radius!r}")
    if not (np.isfinite(r2) and r2 > 0):
        raise ValueError(f"radius squared must be finite and > 0 in float32, got {radius!r}")
    return r


def _check_points(X, name: str) -> torch.Tensor:
    if not (isinstance(X, torch.Tensor) and X.is_cuda):
        raise _lib.PcmError(f"local_moments expects HIP device tensors (no CPU fallback): {name} is not one")
    if X.dim() != 2 or X.shape[1] != 3 or X.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 (n, 3) tensor in z, y, x order")
    if X.shape[0] >= 1 << 31:
        raise ValueError(f"{name} must hold fewer than 2^31 rows")
    return X.contiguous()


def bound(r, q: int) -> int:
    """B = floor(float64(r) (1 + 2^-20) 2^q) + 1 >= |dq| of every pair within r (DESIGN.md §4 "Local moments")."""
    mant, e = math.frexp(float(np.float32(r)) * (1.0 + 2.0 ** -20))
    mant, e = int(math.ldexp(mant, 53)), e - 53 + int(q)
    return (mant << e if e >= 0 else mant >> -e) + 1


def q_cap(m: int, r) -> int:
    """The largest q in [Q_MIN, Q_MAX] with max(m, 1) B(q)^2 <= 2^62 and B(q) < 2^31."""
    rows = max(int(m), 1)
    for q in range(Q_MAX, Q_MIN - 1, -1):
        b = bound(r, q)
        if rows * b * b <= 1 << 62 and b < 1 << 31:
            return q
    raise ValueError(f"no fixed-point exponent q in [{Q_MIN}, {Q_MAX}] keeps the sums of {rows} targets within radius "
                     f"{float(r)!r} in int64")


def default_q(maxabs: Sequence[float], m: int, r) -> Tuple[int, int, int]:
    """``min(fixed_q(maxabs)[a], q_cap(m, r))`` per axis; ``maxabs``: max |coordinate| over the finite rows of both clouds."""
    cap = q_cap(m, r)
    return tuple(max(min(int(v), cap), Q_MIN) for v in fixed_q(maxabs))


def check_q(q, maxabs: Sequence[float], m: int, r) -> Tuple[int, int, int]:
    """The two conditions under which no sum overflows -> q as three ints, or ValueError naming q."""
    try:
        q = tuple(int(v) for v in q)
    except (TypeError, ValueError):
        raise ValueError(f"q must be three integers (z, y, x), got {q!r}") from None
    if len(q) != 3 or any(not Q_MIN <= v <= Q_MAX for v in q):
        raise ValueError(f"q must be three integers in [{Q_MIN}, {Q_MAX}], got {q!r}")
    rows = max(int(m), 1)
    b = [bound(r, v) for v in q]
    if max(b) >= 1 << 31 or rows * max(b) ** 2 > 1 << 62:
        raise ValueError(f"q = {q} is too fine: the int64 sums of up to {rows} targets within radius {float(r)!r} could "
                         f"overflow (m B_a B_b <= 2^62 with B = {b}); the largest safe q is {q_cap(m, r)}")
    for a, v in enumerate(q):
        if not math.ldexp(float(maxabs[a]), v) < 2.0 ** 31:
            raise ValueError(f"q = {q} is too fine: |coordinate| 2^q reaches 2^31 on axis {a} (max |coordinate| "
                             f"{float(maxabs[a])!r})")
    return q


def _maxabs(X: torch.Tensor, Y: Optional[torch.Tensor]) -> np.ndarray:
    """max |coordinate| per axis over the finite rows of the clouds, on the host (float64)."""
    out = torch.zeros(3, dtype=torch.float32, device=X.device)
    for c in (X, Y):
        if c is not None and c.shape[0]:
            fin = torch.isfinite(c).all(dim=1, keepdim=True)
            out = torch.maximum(out, torch.where(fin, c.abs(), torch.zeros_like(c)).amax(0))
    return out.double().cpu().numpy()


def workspace(m: int, device) -> torch.Tensor:
    nbytes = ctypes.c_size_t()
    _lib.check(_lib.load().pcm_moments_workspace(int(m), ctypes.byref(nbytes)), "pcm_moments_workspace")
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def moments_scan(X: torch.Tensor, Y: Optional[torch.Tensor], r: np.float32, q, xskeys, xperm, yskeys, yperm,
                 info: torch.Tensor, ws: Optional[torch.Tensor], words: torch.Tensor) -> None:
    """``pcm_moments_scan`` on checked arguments (``Y`` None: the targets are the queries): stream-ordered."""
    from .engine import _ptr, _stream

    def ptr(t):
        return _ptr(t) if t is not None and t.numel() else None

    q3 = (ctypes.c_int32 * 3)(*[int(v) for v in q])
    rc = _lib.load().pcm_moments_scan(ptr(X), int(X.shape[0]), ptr(Y), int(Y.shape[0]) if Y is not None else 0,
                                      ctypes.c_float(float(r)), q3, ptr(xskeys), ptr(xperm), ptr(yskeys), ptr(yperm),
                                      ptr(words), _ptr(info), ptr(ws), int(ws.numel()) if ws is not None else 0, _stream())
    _lib.check(rc, "pcm_moments_scan")


def local_moments(X: torch.Tensor, radius: float, *, targets: Optional[torch.Tensor] = None, q=None) -> LocalMoments:
    """For every row (z, y, x) of ``X`` (n, 3) the exact moments of the rows of ``targets`` (m, 3) within ``radius``.

    Target j is in the neighbourhood of query i iff both rows are finite and ``(dz*dz + dy*dy) +
    dx*dx <= r*r`` in float32 (r = float32(radius), differences X[i] - Y[j], no FMA):
    ``nearest_points``' predicate.  ``targets=None`` means ``X`` itself; a row is then in its own
    neighbourhood, so ``counts() == radius_support(X, radius).counts + 1`` on the finite rows.
    With ``dq_a = trunc(ldexp(Y[j,a], q_a)) - trunc(ldexp(X[i,a], q_a))``, ``words[i]`` holds the
    count, the three sums of ``dq_a`` and the six sums of ``dq_a dq_b`` (zz, zy, zx, yy, yx, xx)
    over the neighbourhood, as int64: integer sums, bit for bit one answer for any row order.  A
    query with a NaN or Inf coordinate gets ten zeros (``skipped``); such a target is in no
    neighbourhood (``skipped_targets``).

    ``q``: the fixed-point exponents (z, y, x).  The default is ``fixed_q`` of max |coordinate| over
    both clouds, capped so that no sum can overflow: with ``B = floor(r (1 + 2^-20) 2^q) + 1``
    (no pair within the radius has a larger ``|dq|``), ``max(m, 1) B_a B_b <= 2^62``.  A ``q`` that
    breaks this, or with ``|coordinate| 2^q >= 2^31``, raises ValueError.

    The scan tests a query against every target of the cells around it: its cost grows with the
    product of the cells' populations (DESIGN.md §4 "Local moments").
    """
    X = _check_points(X, "X")
    Y = None if targets is None or targets is X else _check_points(targets, "targets")
    if Y is not None and Y.device != X.device:
        raise ValueError("X and targets must be on the same device")
    n = int(X.shape[0])
    m = n if Y is None else int(Y.shape[0])
    r = _radius32(radius)
    maxabs = _maxabs(X, Y)
    q = default_q(maxabs, m, r) if q is None else check_q(q, maxabs, m, r)
    words = torch.zeros((n, _lib.MOMENTS_WORDS), dtype=torch.int64, device=X.device)
    xkeys, ykeys, info = nearest_keys(X, X[:0] if Y is None else Y, r)
    if n and m:
        xskeys, xperm = torch.sort(xkeys)
        yskeys, yperm = (None, None) if Y is None else torch.sort(ykeys)
        moments_scan(X, Y, r, q, xskeys, xperm, yskeys, yperm, info, workspace(m, X.device), words)
    host = info.tolist()
    if host[I_BADPERM]:
        raise _lib.PcmError("local_moments: a sort did not return a permutation")
    skipped = int(host[I_SKIPPED])
    return LocalMoments(words=words, q=q, radius=float(r), skipped=skipped,
                        skipped_targets=skipped if Y is None else int(host[I_SKIPPED_TARGETS]), cell_log2=int(host[0]))


def moments_planes(words: torch.Tensor, q, min_count: int):
    """``pcm_moments_planes`` on checked arguments -> (normal (n, 3), distance, roughness, planarity), float32, device."""
    from .engine import _ptr, _stream
    n = int(words.shape[0])
    normal = torch.empty((n, 3), dtype=torch.float32, device=words.device)
    distance, roughness, planarity = (torch.empty(n, dtype=torch.float32, device=words.device) for _ in range(3))
    q3 = (ctypes.c_int32 * 3)(*[int(v) for v in q])
    rc = _lib.load().pcm_moments_planes(_ptr(words) if n else None, n, q3, int(min_count), _ptr(normal) if n else None,
                                        _ptr(distance) if n else None, _ptr(roughness) if n else None,
                                        _ptr(planarity) if n else None, _stream())
    _lib.check(rc, "pcm_moments_planes")
    return normal, distance, roughness, planarity


def _min_count(min_count) -> int:
    if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or min_count < 0:
        raise ValueError(f"min_count must be an integer >= 0, got {min_count!r}")
    return int(min_count)


def point_normals(X: torch.Tensor, radius: float, *, targets: Optional[torch.Tensor] = None, min_count: int = 3, q=None,
                  moments: Optional[LocalMoments] = None) -> PointNormals:
    """The plane through the rows of ``targets`` (default: ``X`` itself) within ``radius`` of every row of ``X``.

    From ``local_moments(X, radius, targets=, q=)`` -- or ``moments``, the result of that very call
    -- in float64 on the device: the mean offset ``mu`` and the covariance ``C`` of the
    neighbourhood, the eigenvalues ``l0 <= l1 <= l2`` of ``C`` by cyclic Jacobi.  ``normal`` is the
    unit eigenvector of ``l0``, signed as in ``surface_elements`` (z >= 0, ties by y then x; a
    component within 2^-30 of 0 is set to 0 first, so a vertical plane's sign comes from y, not from noise);
    ``roughness = sqrt(max(l0, 0))``; ``planarity = (l1 - l0) / l2``, 0 where ``l2 <= 0``;
    ``distance = -normal . mu``, the signed distance of the row to the plane through the
    neighbourhood's mean, positive when the row lies on the +z side: with ``targets`` an earlier
    day, the change along the surface normal (point-to-plane).  All float32.  Rows with fewer than
    ``max(min_count, 1)`` targets within the radius are NaN.  Where the two smallest eigenvalues
    coincide (collinear or isotropic neighbourhoods) the normal is one of many.
    """
    min_count = _min_count(min_count)
    if moments is None:
        moments = local_moments(X, radius, targets=targets, q=q)
    else:
        if not isinstance(moments, LocalMoments) or not isinstance(X, torch.Tensor) or \
                tuple(moments.words.shape) != (int(X.shape[0]), _lib.MOMENTS_WORDS):
            raise ValueError(f"moments must be the LocalMoments of this call: words of shape ({int(X.shape[0])}, "
                             f"{_lib.MOMENTS_WORDS})")
        if moments.radius != float(_radius32(radius)) or (q is not None and tuple(int(v) for v in q) != tuple(moments.q)):
            raise ValueError("moments must be the LocalMoments of this call: its radius or q differs")
    normal, distance, roughness, planarity = moments_planes(moments.words.contiguous(), moments.q, min_count)
    return PointNormals(normal=normal, distance=distance, roughness=roughness, planarity=planarity,
                        count=moments.counts(), min_count=min_count, moments=moments)
