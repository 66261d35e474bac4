"""Co-registration of labelled days onto a set of centres, before they are fused.

The reference builds every pair's cloud in that pair's own frame (pixels of its
rectified image, z as the residual of its own plane, shifted by its own 2nd
percentile), so two days differ by a height offset and usually a small tilt and
a pixel shift.  ``register_days`` removes that: nearest-centre Kabsch iterations
in which every pass over the points is ``pcm_align_stats`` (DESIGN.md §4
"Registration: k_align") -- the row is transformed by its day's current motion,
finds its canonical nearest centre, and adds exact fixed-point sums to its day's
38 words -- and every solve is host float64 on O(G) exact integers.  The words
are integers, so they are additive over chunks, clouds and ranks (``out=``,
``+``).  There is no CPU fallback for the pass; the accessors and the solves
work on any words (device tensor or NumPy array).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib
from .fixed import fixed_q

WORDS = _lib.ALIGN_WORDS
KINDS = ("z", "translation", "rigid")
RANK_EPS = 1e-12     # rigid: the second singular value of H must exceed RANK_EPS times the first

_frac = np.frompyfunc(lambda a, b: float(a) / float(b) if b else float("nan"), 2, 1)


def _limbs(w: np.ndarray, first: int, count: int) -> np.ndarray:
    """``count`` lo/hi pairs from word ``first`` on as exact Python ints: object array (G, count)."""
    lo = w[:, first:first + 2 * count:2].view(np.uint64).astype(object)
    hi = w[:, first + 1:first + 2 * count:2].astype(object)
    return lo + hi * (1 << 32)


class AlignStats:
    """The words of ``pcm_align_stats`` for G groups.

    ``words``: int64 (G, 38) -- a device tensor as ``align_stats`` returns it, or a
    NumPy array (int64 / uint64 bit patterns); ``q``: the three fixed-point
    exponents the words were formed with.
    """

    def __init__(self, words, q, _buf=None):
        if not isinstance(words, torch.Tensor):
            words = np.ascontiguousarray(words).view(np.int64) if np.asarray(words).dtype == np.uint64 \
                else np.ascontiguousarray(words, dtype=np.int64)
        if words.ndim != 2 or words.shape[1] != WORDS:
            raise ValueError(f"words must be (G, {WORDS})")
        self.words = words
        self.q = [int(v) for v in q]
        if len(self.q) != 3:
            raise ValueError("q must hold 3 exponents")
        self._buf = _buf     # device: the (G*38 + 1) buffer `words` views; its last word counts skipped rows

    @property
    def n_groups(self) -> int:
        return int(self.words.shape[0])

    def numpy(self) -> np.ndarray:
        """The words on the host, int64 (G, 38)."""
        w = self.words
        return w.cpu().numpy() if isinstance(w, torch.Tensor) else w

    def _same(self, other: "AlignStats"):
        if not isinstance(other, AlignStats) or tuple(other.words.shape) != tuple(self.words.shape) or other.q != self.q:
            raise ValueError("AlignStats differ in shape or q")

    # ------------------------------------------------------------ exact
    def inliers(self) -> np.ndarray:
        return self.numpy()[:, 0].copy()

    def outliers(self) -> np.ndarray:
        return self.numpy()[:, 1].copy()

    def sums_p(self) -> np.ndarray:
        """sum pq_a over the inliers, int64 (G, 3)."""
        return self.numpy()[:, 2:5].copy()

    def sums_c(self) -> np.ndarray:
        return self.numpy()[:, 5:8].copy()

    def cross(self) -> np.ndarray:
        """sum pq_a cq_b as exact Python ints: object array (G, 3, 3)."""
        return _limbs(self.numpy(), 8, 9).reshape(-1, 3, 3)

    def sq_p(self) -> np.ndarray:
        """sum pq_a^2 as exact Python ints: object array (G, 3)."""
        return _limbs(self.numpy(), 26, 3)

    def sq_c(self) -> np.ndarray:
        return _limbs(self.numpy(), 32, 3)

    def merged(self) -> "AlignStats":
        """The sum over the groups, as a one-group AlignStats."""
        w = self.words
        if isinstance(w, torch.Tensor):
            return AlignStats(w.sum(0, keepdim=True), self.q)
        with np.errstate(over="ignore"):
            return AlignStats(w.view(np.uint64).sum(0, keepdims=True, dtype=np.uint64), self.q)

    def __add__(self, other: "AlignStats") -> "AlignStats":
        self._same(other)
        a, b = self.words, other.words
        if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
            return AlignStats(a + b.to(a.device), self.q)
        with np.errstate(over="ignore"):
            return AlignStats(self.numpy().view(np.uint64) + other.numpy().view(np.uint64), self.q)

    # ------------------------------------------------------------ derived (float64 of exact integer numerators)
    def _means(self):
        n = self.inliers().astype(object)[:, None]
        scale = np.ldexp(1.0, -np.asarray(self.q, dtype=np.int64))
        return (_frac(self.sums_p().astype(object), n).astype(np.float64) * scale,
                _frac(self.sums_c().astype(object), n).astype(np.float64) * scale)

    def rms(self) -> np.ndarray:
        """Per group, the rms distance of the inliers to their centres:
        sqrt(sum_a 2^(-2 q_a) (P_a + C_a - 2 M_aa) / n); NaN without inliers."""
        n = self.inliers().astype(object)
        M = self.cross()
        num = self.sq_p() + self.sq_c() - 2 * np.stack([M[:, a, a] for a in range(3)], axis=1)   # exact, >= 0
        per_axis = np.ldexp(_frac(num, n[:, None]).astype(np.float64), -2 * np.asarray(self.q, dtype=np.int64))
        return np.sqrt(per_axis.sum(1))

    def solve(self, kind: str = "rigid"):
        """The motion that best maps each group's inliers onto their centres, least squares:
        (R (G, 3, 3), t (G, 3), ok (G,)) float64, c ~ R p + t.

        ``"z"``: t_0 = mean c_0 - mean p_0 only; ``"translation"``: t = mean c - mean p;
        ``"rigid"``: Kabsch on H = M - S_p S_c^T / n, whose numerator n M - S_p (x) S_c is
        formed in Python ints: R = V diag(1, 1, det(V U^T)) U^T, t = mean c - R mean p.  A
        group with fewer than 3 inliers or an H of rank below 2 falls back to the translation
        (ok False); one without inliers keeps the identity (ok False)."""
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        G = self.n_groups
        n = self.inliers()
        pm, cm = self._means()
        R = np.tile(np.eye(3), (G, 1, 1))
        t = np.zeros((G, 3))
        ok = n > 0
        have = np.flatnonzero(n > 0)
        if kind == "z":
            t[have, 0] = cm[have, 0] - pm[have, 0]
            return R, t, ok
        t[have] = cm[have] - pm[have]
        if kind == "translation":
            return R, t, ok
        no = n.astype(object)[:, None, None]
        Sp, Sc = self.sums_p().astype(object), self.sums_c().astype(object)
        num = no * self.cross() - Sp[:, :, None] * Sc[:, None, :]
        q = np.asarray(self.q, dtype=np.int64)
        H = np.ldexp(_frac(num, no * no).astype(np.float64), -(q[:, None] + q[None, :]))
        ok = ok.copy()
        for g in range(G):
            if n[g] < 3:
                ok[g] = False
                continue
            U, S, Vt = np.linalg.svd(H[g])
            if not S[1] > RANK_EPS * S[0]:
                ok[g] = False
                continue
            V = Vt.T
            d = 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0
            R[g] = V @ np.diag([1.0, 1.0, d]) @ U.T
            t[g] = cm[g] - R[g] @ pm[g]
        return R, t, ok


# ---------------------------------------------------------------- the pass
def pack_transforms(R, t) -> np.ndarray:
    """(G, 3, 3), (G, 3) -> the (G, 12) float32 rows the kernel reads: R row-major, then t."""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([R.reshape(-1, 9), t], axis=1).astype(np.float32))


def default_q(xabs, cabs, transforms=None) -> list:
    """``fixed_q`` over the centres (``cabs``: max |c_a|) and the per-axis bound
    sum_b |R_ab| max|x_b| + |t_a| of the transformed points, taken over the groups
    (a 2^-20 slack covers the float32 roundings of the transform)."""
    xabs = np.asarray(xabs, dtype=np.float64)
    if transforms is None:
        bound = xabs
    else:
        T = np.abs(np.asarray(transforms, dtype=np.float64).reshape(-1, 12))
        bound = ((T[:, :9].reshape(-1, 3, 3) * xabs[None, None, :]).sum(2) + T[:, 9:]).max(0) * (1.0 + 2.0 ** -20)
    return fixed_q(np.maximum(bound, np.asarray(cabs, dtype=np.float64)))


class AlignPlan:
    """A prepared registration workspace: the centres' pruning grid and exact candidate lists
    (``pcm_align_prepare``), built once and reused by every ``align_stats`` call on these centres."""

    def __init__(self, centers: torch.Tensor, n_hint: int, max_dist: Optional[float] = None):
        if not (isinstance(centers, torch.Tensor) and centers.is_cuda):
            raise _lib.PcmError("align expects device tensors (no CPU fallback)")
        if centers.dim() != 2 or centers.shape[1] != 3 or centers.shape[0] < 1 or centers.dtype != torch.float32:
            raise ValueError("centers must be a float32 (K, 3) tensor")
        from .engine import _ptr, _stream
        self.centers = centers.contiguous()
        self.k = int(centers.shape[0])
        self.n_hint = max(int(n_hint), 1)
        self.max_d2 = _max_d2(max_dist)
        lib = _lib.load()
        nbytes = ctypes.c_size_t()
        _lib.check(lib.pcm_align_workspace(self.n_hint, self.k, ctypes.byref(nbytes)), "pcm_align_workspace")
        self.ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=centers.device)
        self.plan = _lib.PcmAlignPlan()
        info = (ctypes.c_int64 * 3)()
        _lib.check(lib.pcm_align_prepare(_ptr(self.centers), self.k, self.n_hint, ctypes.c_float(self.max_d2),
                                         _ptr(self.ws), int(nbytes.value), ctypes.byref(self.plan), info, _stream()),
                   "pcm_align_prepare")
        self.info = dict(cells=int(info[0]), full_cells=int(info[1]), list_total=int(info[2]))
        c = self.centers.cpu().numpy()
        self.cabs = np.abs(c).max(0).astype(np.float64)
        self.half_diagonal = 0.5 * float(np.linalg.norm(c.max(0).astype(np.float64) - c.min(0).astype(np.float64)))


def _max_d2(max_dist) -> float:
    """The float32 bound the kernel compares d2 with: fl32(max_dist)^2 rounded to float32; None: +inf."""
    if max_dist is None:
        return math.inf
    m = np.float32(max_dist)
    if not m >= 0:
        raise ValueError(f"max_dist must be >= 0 or None, got {max_dist!r}")
    with np.errstate(over="ignore"):
        return float(np.float32(m * m))


def _groups8(groups, n: int, n_groups, default_g, device):
    if groups is None:
        G = int(n_groups) if n_groups is not None else default_g(1)
        g8 = None
    else:
        if not (isinstance(groups, torch.Tensor) and groups.is_cuda and tuple(groups.shape) == (n,)) or \
                groups.dtype.is_floating_point or groups.dtype == torch.bool:
            raise ValueError(f"groups must be an integer device tensor of shape ({n},)")
        lo, hi = (int(groups.min()), int(groups.max())) if n else (0, 0)
        G = int(n_groups) if n_groups is not None else default_g(hi + 1)
        if lo < 0 or hi >= G:
            raise ValueError(f"groups must lie in [0, {G}); found [{lo}, {hi}]")
        g8 = groups.to(torch.uint8).contiguous()
    if not 1 <= G <= _lib.ALIGN_MAXG:
        raise ValueError(f"n_groups must be 1..{_lib.ALIGN_MAXG}, got {G}")
    return g8, G


def _check_points(X, what: str):
    if not (isinstance(X, torch.Tensor) and X.is_cuda):
        raise _lib.PcmError(f"{what} expects a HIP device tensor (no CPU fallback)")
    if X.dim() != 2 or X.shape[1] != 3 or X.dtype != torch.float32:
        raise ValueError("X must be a float32 (n, 3) tensor in z, y, x order")
    return X.contiguous()


def _xabs(X: torch.Tensor) -> np.ndarray:
    """max |x_a| over the finite coordinates (a NaN or Inf row is skipped by the pass, and reported)."""
    if not X.shape[0]:
        return np.zeros(3)
    return torch.where(torch.isfinite(X), X.abs(), torch.zeros_like(X)).amax(0).double().cpu().numpy()


def _transforms32(transforms, G: int) -> np.ndarray:
    T = np.ascontiguousarray(np.asarray(transforms, dtype=np.float32).reshape(-1, 12))
    if T.shape[0] != G:
        raise ValueError(f"transforms must hold {G} rows of 12 floats (R row-major, then t)")
    if not np.isfinite(T).all():
        raise ValueError("transforms contain NaN or Inf")
    return T


def accumulate(X: torch.Tensor, groups8: Optional[torch.Tensor], n_groups: int, T: Optional[torch.Tensor], max_d2: float,
               qa: np.ndarray, buf: torch.Tensor, plan: AlignPlan) -> None:
    """``pcm_align_stats`` on checked arguments: adds the rows' words into ``buf`` (device int64,
    n_groups * 38 + 1), stream-ordered, without any synchronisation (``groups8``: uint8 or None;
    ``T``: device float32 (G, 12) or None)."""
    from .engine import _ptr, _stream
    n = int(X.shape[0])
    rc = _lib.load().pcm_align_stats(_ptr(X) if n else None, n, _ptr(groups8) if (groups8 is not None and n) else None,
                                     n_groups, _ptr(T) if T is not None else None, ctypes.c_float(max_d2),
                                     qa.ctypes.data_as(ctypes.c_void_p), _ptr(buf), None, _ptr(plan.ws),
                                     ctypes.byref(plan.plan), _stream())
    _lib.check(rc, "pcm_align_stats")


def align_stats(X: torch.Tensor, centers: torch.Tensor, *, groups: Optional[torch.Tensor] = None,
                n_groups: Optional[int] = None, transforms=None, max_dist: Optional[float] = None, q=None,
                out: Optional[AlignStats] = None, plan: Optional[AlignPlan] = None) -> AlignStats:
    """One ``pcm_align_stats`` pass over the rows of ``X`` (n, 3) float32 (z, y, x) on the device.

    ``centers``: device float32 (K, 3).  ``groups``: any integer device tensor (n,)
    with values in [0, n_groups) -- the day of each row (default: one group);
    ``n_groups`` (<= 256) defaults to ``max + 1``.  ``transforms``: (G, 12) or
    None -- each group's R (row-major) and t, applied in float32 before the
    search.  ``max_dist``: rows farther than this from their nearest centre are
    counted as outliers and add nothing else (None: no trimming).  ``q``: the
    fixed-point exponents, default ``default_q`` of this cloud, these centres and
    these transforms.  ``out``: an earlier result of the same (G, q) to accumulate
    into; fewer than 2^31 rows in all may go into one result.  ``plan``: an
    ``AlignPlan`` of these centres (built here when None; a driver reuses one).
    Raises ValueError when rows were skipped (group out of range, NaN or Inf, or a
    transformed point beyond the fixed-point range of ``q``).
    """
    from .engine import _ptr, _stream
    X = _check_points(X, "align_stats")
    n = int(X.shape[0])
    if plan is None:
        plan = AlignPlan(centers, n, max_dist)
    elif not isinstance(plan, AlignPlan) or plan.ws.device != X.device:
        raise ValueError("plan must be an AlignPlan on the device of X")
    g8, G = _groups8(groups, n, n_groups, lambda d: out.n_groups if out is not None else d, X.device)
    T = None if transforms is None else _transforms32(transforms, G)
    if q is None:
        q = out.q if out is not None else \
            default_q(_xabs(X), plan.cabs, T)
    qa = np.ascontiguousarray(np.asarray(q, dtype=np.int32))
    if qa.shape != (3,):
        raise ValueError("q must hold 3 exponents")
    if out is None:
        buf = torch.zeros(G * WORDS + 1, dtype=torch.int64, device=X.device)
        out = AlignStats(buf[:-1].view(G, WORDS), qa.tolist(), _buf=buf)
    else:
        if not isinstance(out, AlignStats) or out._buf is None or out._buf.device != X.device:
            raise ValueError("out must be an AlignStats that align_stats returned on this device")
        if (out.n_groups, out.q) != (G, qa.tolist()):
            raise ValueError("out differs in (n_groups, q)")
    accumulate(X, g8, G, None if T is None else torch.from_numpy(T).to(X.device), _max_d2(max_dist), qa, out._buf, plan)
    skipped = int(out._buf[-1])
    if skipped:
        raise ValueError(f"align_stats skipped {skipped} rows (group out of range, NaN or Inf, or beyond the range of q)")
    return out


# ---------------------------------------------------------------- the driver
@dataclass
class Registration:
    R: np.ndarray            # (G, 3, 3) float64
    t: np.ndarray            # (G, 3) float64
    ok: np.ndarray           # (G,) bool: every solve of the group was of the kind asked for
    n_iter: int
    converged: bool
    inliers: np.ndarray      # (G,) int64, at the final transforms
    outliers: np.ndarray
    rms_before: np.ndarray   # (G,) rms distance of the inliers to their centres at the initial transforms
    rms_after: np.ndarray    # ... at the final ones
    transforms: np.ndarray   # (G, 12) float32: what the kernel applied (R row-major, then t)

    def as_dict(self) -> dict:
        return dict(R=self.R, t=self.t, ok=self.ok, n_iter=int(self.n_iter), converged=bool(self.converged),
                    inliers=self.inliers, outliers=self.outliers, rms_before=self.rms_before,
                    rms_after=self.rms_after, transforms=self.transforms)


def register_loop(stats_fn: Callable[[np.ndarray], AlignStats], n_groups: int, half_diagonal: float, *,
                  kind: str = "rigid", max_iter: int = 50, tol: float = 1e-3, init=None) -> Registration:
    """The registration driver over any statistics pass: ``stats_fn(T)`` returns the AlignStats of
    the cloud under the (G, 12) float32 transforms ``T``.  Each iteration solves for the
    increment (R_d, t_d) and composes R <- R_d R, t <- R_d t + t_d in float64; it stops when, for
    every group, |t_d|_inf <= tol and ||R_d - I||_F * half_diagonal <= tol."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    G = int(n_groups)
    if init is None:
        R, t = np.tile(np.eye(3), (G, 1, 1)), np.zeros((G, 3))
    else:
        T0 = np.asarray(init.transforms if isinstance(init, Registration) else init, dtype=np.float64).reshape(-1, 12)
        if T0.shape[0] != G:
            raise ValueError(f"init must hold {G} transforms")
        R, t = T0[:, :9].reshape(G, 3, 3).copy(), T0[:, 9:].copy()
    ok = np.ones(G, dtype=bool)
    rms_before, n_iter, converged = None, 0, False
    st = stats_fn(pack_transforms(R, t))
    for _ in range(int(max_iter)):
        if rms_before is None:
            rms_before = st.rms()
        Rd, td, okd = st.solve(kind)
        ok &= okd
        R = np.einsum("gab,gbc->gac", Rd, R)
        t = np.einsum("gab,gb->ga", Rd, t) + td
        n_iter += 1
        st = stats_fn(pack_transforms(R, t))
        if np.all(np.abs(td).max(1) <= tol) and \
                np.all(np.linalg.norm((Rd - np.eye(3)).reshape(G, 9), axis=1) * half_diagonal <= tol):
            converged = True
            break
    rms_after = st.rms()
    return Registration(R=R, t=t, ok=ok & (st.inliers() > 0), n_iter=n_iter, converged=converged,
                        inliers=st.inliers(), outliers=st.outliers(),
                        rms_before=rms_after if rms_before is None else rms_before, rms_after=rms_after,
                        transforms=pack_transforms(R, t))


def register_days(X: torch.Tensor, centers: torch.Tensor, *, groups: Optional[torch.Tensor] = None,
                  n_groups: Optional[int] = None, kind: str = "rigid", max_dist: Optional[float] = None,
                  max_iter: int = 50, tol: float = 1e-3, init=None) -> Registration:
    """Register every group (day) of the cloud ``X`` (n, 3) onto ``centers`` (K, 3): nearest-centre
    iterations of ``kind`` (``"z"``: a height offset, ``"translation"``, ``"rigid"``), one
    ``align_stats`` pass each over lists prepared once.  ``max_dist`` trims rows farther than that
    from every centre (off by default: trimming below the cells' radius biases the result).
    ``init``: a Registration or (G, 12) transforms to start from.  ``tol`` is in the units of X."""
    X = _check_points(X, "register_days")
    n = int(X.shape[0])
    plan = AlignPlan(centers, n, max_dist)
    g8, G = _groups8(groups, n, n_groups, lambda d: d, X.device)
    xabs = _xabs(X)

    max_d2 = _max_d2(max_dist)

    def stats_fn(T):
        # the arguments were checked above: the bare pass, then one read-back of the 38 G + 1 words
        q = default_q(xabs, plan.cabs, T)
        buf = torch.zeros(G * WORDS + 1, dtype=torch.int64, device=X.device)
        accumulate(X, g8, G, torch.from_numpy(_transforms32(T, G)).to(X.device), max_d2,
                   np.ascontiguousarray(np.asarray(q, dtype=np.int32)), buf, plan)
        host = buf.cpu().numpy()
        if host[-1]:
            raise ValueError(f"register_days skipped {int(host[-1])} rows (NaN or Inf, or beyond the range of q)")
        return AlignStats(host[:-1].reshape(G, WORDS), q)

    return register_loop(stats_fn, G, plan.half_diagonal, kind=kind, max_iter=max_iter, tol=tol, init=init)


def apply_registration(X: torch.Tensor, reg_or_transforms, groups: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The rows of ``X`` under their group's transform, with the arithmetic of the pass
    (``pcm_align_apply``): ``align_stats(apply_registration(X, T))`` equals
    ``align_stats(X, transforms=T)`` bit for bit."""
    from .engine import _ptr, _stream
    X = _check_points(X, "apply_registration")
    n = int(X.shape[0])
    T = reg_or_transforms.transforms if isinstance(reg_or_transforms, Registration) else reg_or_transforms
    T = np.ascontiguousarray(np.asarray(T, dtype=np.float32).reshape(-1, 12))
    g8, G = _groups8(groups, n, T.shape[0], lambda d: d, X.device)
    T = _transforms32(T, G)
    out = torch.empty_like(X)
    Td = torch.from_numpy(T).to(X.device)
    rc = _lib.load().pcm_align_apply(_ptr(X) if n else None, n, _ptr(g8) if (g8 is not None and n) else None, G,
                                     _ptr(Td), _ptr(out) if n else None, _stream())
    _lib.check(rc, "pcm_align_apply")
    return out
