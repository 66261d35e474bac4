"""Drop-in "Multi-day 3D Point Cloud" plugin with the GPU K-means fusion step.

Boundary: the reference's ``HeightMapExtractor``
(members/rafael/disparity/plugin.py:22-243) builds one point cloud per stereo
pair -- ``points_coords = stack([z, y, x])`` (plugin.py:191-192) emitted as a
napari points layer (plugin.py:220-233) -- and never fuses days.  This class
keeps that component's public contract:

* ``name == "Multi-day 3D Point Cloud"`` (plugin.py:32-34; viewer.py:475-476
  dispatches the rafael tab on ``"3D Point Cloud" in plugin.name``);
* ``requires_image = False`` (plugin.py:29-30, read by viewer.py:107);
* ``run(kml_path, is_debug_mode=True, is_debug_pair=False,
  is_one_random_pair=True, n=10)`` (plugin.py:36-40, defaults from
  constants.py:5-10), called on a napari worker thread (widget.py:144-147);
* returns host numpy layers only, and never raises: failures come back as the
  reference's error image layers -- ``np.zeros((100, 100))`` named
  ``"error: image not found"`` / ``"error: <msg>"`` for a missing image or a
  failed crop (plugin.py:77-79, 89-91), otherwise ``np.ones((100, 100))`` named
  ``"Error: <msg>"`` (plugin.py:236-241); the stages write the run log
  ``TEMP/log.txt`` (plugin.py:49-50, 234, 240).

``run`` replays the reference's per-pair stereo stages (``pipeline.py``:
pair selection, crop, ASP rectification, SGBM/WLS disparity -- the reference's
own functions), assembles every pair's cloud ON THE GPU (``plugin.py:147-192``
-> ``cloud.assemble_cloud_device``), emits the reference's per-pair layers
(``plugin.py:176-233``) and appends the fused result of the K-means step that
slots in after plugin.py:192: a centroid points layer and the fused cloud with
a per-point ``cluster`` property.  The device clouds feed the K-means
(``pcm_amd.lloyd_fit``) without a host round trip.  ``base=`` keeps the older
mode: run an extractor with the reference's ``run`` and fuse the cloud layers
it returns.  Extra knobs (K, iterations, tolerance, export) are constructor
arguments so ``run``'s signature stays the reference's (viewer.py:118-127 would
turn extra ``run`` parameters into file pickers).
"""
from __future__ import annotations

import threading
from typing import Callable, List, Optional, Sequence

import numpy as np

try:  # inside the reference tree: the real plugin ABC
    from interface import SatellitePlugin  # type: ignore
except Exception:  # headless / tests
    from ._interface import SatellitePlugin

from .fixed import fixed_q

PREFIX = "[Multi-day 3D Point Cloud]"
CLOUD_LAYER_SUFFIX = "3D Point Cloud"
DEFAULTS = dict(is_debug_mode=True, is_debug_pair=False, is_one_random_pair=True, n=10)

_gpu_lock = threading.Lock()   # one fit at a time per process (widgets may run concurrently)


def _tolerance(X: np.ndarray, tol: float) -> float:
    """sklearn ``_tolerance`` (_kmeans.py:279-287): mean per-axis variance x tol."""
    if tol == 0 or X.shape[0] == 0:
        return 0.0
    return float(np.mean(np.var(X.astype(np.float64), axis=0)) * tol)


def _gpu_fit(X, C0: np.ndarray, max_iter: int, tol_abs: float):
    """X: host (N, 3) array, or the fused cloud already on the device."""
    import torch

    from .lloyd import LOCAL, lloyd_fit

    with _gpu_lock:
        Xt = X.to(torch.float32).contiguous() if isinstance(X, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
        Ct = torch.from_numpy(np.ascontiguousarray(C0, dtype=np.float32)).cuda()
        res = lloyd_fit(Xt, Ct, max_iter=max_iter, tol=tol_abs, group=LOCAL)   # whole cloud, this GPU
        torch.cuda.synchronize()
        return (res.labels.cpu().numpy(), res.centers.cpu().numpy(), float(res.inertia), int(res.n_iter))


def _norm(v: np.ndarray) -> np.ndarray:
    """Height property as the reference builds it: 2/98 percentiles -> [0, 1] (plugin.py:181-188)."""
    if v.size == 0:
        return v.astype(np.float64)
    lo, hi = np.percentile(v, 2), np.percentile(v, 98)
    return np.clip((v - lo) / (hi - lo + 1e-6), 0.0, 1.0)


def _gpu_kpp(X, k: int, seed: int) -> np.ndarray:
    import torch

    from .kpp import kmeans_plusplus

    with _gpu_lock:
        Xt = X.to(torch.float32).contiguous() if isinstance(X, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
        C, _ = kmeans_plusplus(Xt, k, random_state=seed)
        return C.cpu().numpy()


def export_fused(path, points: np.ndarray, result: dict):
    """On-disk fused cloud (row f4), the analogue of the reference's per-pair
    ``np.savez_compressed(path + 'consistency', ...)`` (disparity.py:220-224):
    fused (N, 3) z,y,x points (float64), per-point ``cluster`` labels, the (K, 3)
    centres, per-cluster counts, inertia and iterations.  ``load_fused`` reads it back."""
    np.savez_compressed(path, points=np.asarray(points, dtype=np.float64), cluster=result["labels"].astype(np.int32),
                        centers=np.asarray(result["centers"], dtype=np.float64),
                        counts=np.bincount(result["labels"], minlength=len(result["centers"])),
                        inertia=np.float64(result["inertia"]), n_iter=np.int64(result["n_iter"]))


def load_fused(path) -> dict:
    with np.load(path, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _gpu_stats(X, labels: np.ndarray, groups: np.ndarray, k: int, n_groups: int) -> np.ndarray:
    """X: host (N, 3) float32 array, or the cloud already on the device -> the words (G, K, 16) as NumPy,
    formed with the exponents ``fixed_q(max|X|)`` of that cloud."""
    import torch

    from .stats import cluster_stats

    with _gpu_lock:
        Xt = X.to(torch.float32).contiguous() if isinstance(X, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
        q = fixed_q(Xt.abs().amax(0).cpu().numpy())
        st = cluster_stats(Xt, torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(Xt.device), k,
                           groups=torch.from_numpy(np.ascontiguousarray(groups, dtype=np.uint8)).to(Xt.device),
                           n_groups=n_groups, q=q)
        return st.numpy()


def _describe(X: np.ndarray, labels: np.ndarray, sizes, k: int, Xdev, stats: Optional[Callable]):
    """The exact per-(cloud, cluster) moments of the labelled cloud (``stats.ClusterStats`` on host words)."""
    from .stats import ClusterStats
    groups = np.repeat(np.arange(len(sizes), dtype=np.uint8), sizes)
    words = (stats or _gpu_stats)(Xdev, np.asarray(labels, dtype=np.int32), groups, k, len(sizes))
    return ClusterStats(np.asarray(words), fixed_q(np.abs(X).max(axis=0)), 3)


GRID_LIMIT_BYTES = 1 << 32     # the words of a fused height map: 32 B per (cloud, pixel)


def _gpu_grid(X, labels: np.ndarray, groups: np.ndarray, k: int, n_groups: int, shape, cell_log2: int, q: int):
    """X: host (N, 3) float32 array, or the cloud already on the device -> the words (G, 4, H, W) as NumPy
    and the number of rows outside the raster (origin (0, 0))."""
    import torch

    from .grid import height_grid

    with _gpu_lock:
        Xt = X.to(torch.float32).contiguous() if isinstance(X, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
        hg = height_grid(Xt, shape, cell_log2=cell_log2, q=q, n_clusters=k, n_groups=n_groups,
                         labels=torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(Xt.device),
                         groups=torch.from_numpy(np.ascontiguousarray(groups, dtype=np.uint8)).to(Xt.device))
        return hg.numpy(), hg.outside


def _height_map(X: np.ndarray, labels: np.ndarray, centers: np.ndarray, sizes, k: int, s: int, Xdev,
                grid: Optional[Callable]):
    """One ``height_grid`` pass over the labelled fused cloud (group = cloud index) -> (image layers, dict)."""
    from .grid import HeightGrid
    s = int(s)
    if not -8 <= s <= 16:
        raise ValueError(f"height_map_cell_log2 must be -8..16, got {s}")
    G = len(sizes)
    # origin (0, 0): the last cell that holds a point, floor(max / 2^s), in the kernel's float32
    far = np.floor(np.ldexp(X[:, 1:].max(axis=0), -s))
    H, W = (max(1, int(v) + 1) for v in far)
    if G * 4 * H * W * 8 > GRID_LIMIT_BYTES or H > 1 << 24 or W > 1 << 24:
        raise ValueError(f"fused height map of {G} clouds on {H} x {W} cells needs {G * 32 * H * W / 2 ** 30:.1f} GiB "
                         f"of words (limit 4 GiB): raise height_map_cell_log2 (now {s})")
    q = fixed_q([np.abs(X[:, 0]).max()])[0]
    groups = np.repeat(np.arange(G, dtype=np.uint8), sizes)
    words, outside = (grid or _gpu_grid)(Xdev, np.asarray(labels, dtype=np.int32), groups, k, G, (H, W), s, q)
    hg = HeightGrid(np.asarray(words), q, s, (0.0, 0.0), outside)
    one = hg.merged()
    present = hg.counts() > 0                                       # (G, H, W)
    mz = hg.means()                                                 # NaN where a cloud has no point
    with np.errstate(invalid="ignore"):
        spread = np.where(present.sum(0) >= 2, np.fmax.reduce(mz, axis=0) - np.fmin.reduce(mz, axis=0), 0.0)
    top = one.top_labels()[0]
    surface = np.where(top >= 0, np.asarray(centers, dtype=np.float64)[np.maximum(top, 0), 0], np.nan)
    scale = (2.0 ** s, 2.0 ** s)
    image = {"colormap": "turbo", "scale": scale}
    layers = [
        (one.means()[0], {"name": f"{PREFIX} Fused Height Map", **image}, "image"),
        (np.nan_to_num(spread, nan=0.0), {"name": f"{PREFIX} Fused Height Spread", **image}, "image"),
        (present.sum(0).astype(np.int32), {"name": f"{PREFIX} Fused Coverage", **image,
                                           "contrast_limits": [0, G]}, "image"),
        (surface, {"name": f"{PREFIX} Fused Surface Height", **image}, "image"),
        ((top + 1).astype(np.int32), {"name": f"{PREFIX} Fused Surface Elements", "scale": scale}, "labels"),
    ]
    return layers, dict(words=hg.numpy(), q=q, cell_log2=s, origin=(0.0, 0.0), shape=(H, W), outside=int(outside),
                        sizes=list(sizes))


REGISTER_KINDS = ("z", "translation", "rigid")


def _gpu_align(X: np.ndarray, C: np.ndarray, groups: np.ndarray, n_groups: int, kind: str, max_dist):
    """Host (N, 3) float32 rows and their cloud index -> (the Registration's fields as a dict, the registered
    rows as float32 NumPy): ``register_days`` onto the centres ``C``, then ``apply_registration``."""
    import torch

    from .align import apply_registration, register_days

    with _gpu_lock:
        Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
        gt = torch.from_numpy(np.ascontiguousarray(groups, dtype=np.uint8)).to(Xt.device)
        Ct = torch.from_numpy(np.ascontiguousarray(C, dtype=np.float32)).to(Xt.device)
        reg = register_days(Xt, Ct, groups=gt, n_groups=n_groups, kind=kind, max_dist=max_dist)
        out = apply_registration(Xt, reg, gt)
        torch.cuda.synchronize()
        return reg.as_dict(), out.cpu().numpy()


def _register_clouds(clouds, centers: np.ndarray, fixed: Optional[int], kind: str, max_dist, align: Optional[Callable]):
    """Register every cloud but ``fixed`` (None: every cloud) onto ``centers``; group = the cloud's index.
    -> (the clouds in the centres' frame (float64 of the float32 the pass wrote), the registration dict
    over ALL clouds: the fixed one keeps the identity, no inliers and NaN rms)."""
    if kind not in REGISTER_KINDS:
        raise ValueError(f"register must be None or one of {REGISTER_KINDS}, got {kind!r}")
    G = len(clouds)
    if G > 256:
        raise ValueError(f"register= takes at most 256 clouds (groups), got {G}")
    moving = [i for i in range(G) if i != fixed]
    reg = dict(R=np.tile(np.eye(3), (G, 1, 1)), t=np.zeros((G, 3)), ok=np.ones(G, dtype=bool), n_iter=0,
               converged=True, inliers=np.zeros(G, dtype=np.int64), outliers=np.zeros(G, dtype=np.int64),
               rms_before=np.full(G, np.nan), rms_after=np.full(G, np.nan),
               transforms=np.tile(np.r_[np.eye(3).ravel(), np.zeros(3)].astype(np.float32), (G, 1)))
    if not moving:
        return list(clouds), reg
    X = np.concatenate([clouds[i] for i in moving]).astype(np.float32)          # boundary cast
    sizes = [clouds[i].shape[0] for i in moving]
    groups = np.repeat(np.arange(len(moving), dtype=np.uint8), sizes)
    part, Xr = (align or _gpu_align)(X, np.ascontiguousarray(centers, dtype=np.float32), groups, len(moving), kind,
                                     max_dist)
    for key in ("R", "t", "ok", "inliers", "outliers", "rms_before", "rms_after", "transforms"):
        reg[key][moving] = np.asarray(part[key])
    reg["n_iter"], reg["converged"] = int(part["n_iter"]), bool(part["converged"])
    out, at = list(clouds), 0
    for i, m in zip(moving, sizes):
        out[i] = np.asarray(Xr[at:at + m], dtype=np.float64)
        at += m
    return out, reg


def _gpu_support(X: np.ndarray, groups: np.ndarray, n_groups: int, radius: float, min_neighbors: int, min_days: int):
    """Host (N, 3) float32 rows and their cloud index -> the bool keep mask of ``filter_outliers``
    (the groups are passed on only when days are asked for)."""
    import torch

    from .support import filter_outliers

    with _gpu_lock:
        Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
        gt = None
        if min_days > 1:
            gt = torch.from_numpy(np.ascontiguousarray(groups, dtype=np.uint8)).to(Xt.device)
        keep = filter_outliers(Xt, radius, min_neighbors, min_days=min_days, groups=gt,
                               n_groups=n_groups if gt is not None else None)
        return keep.cpu().numpy()


def _denoise_args(denoise, days_allowed: bool):
    """(radius, min_neighbors[, min_days]) -> (radius, min_neighbors, min_days), checked."""
    try:
        parts = tuple(denoise)
    except TypeError:
        parts = ()
    if len(parts) not in (2, 3):
        raise ValueError(f"denoise must be None, (radius, min_neighbors) or (radius, min_neighbors, min_days), "
                         f"got {denoise!r}")
    radius, min_neighbors = float(parts[0]), int(parts[1])
    min_days = int(parts[2]) if len(parts) == 3 else 1
    if not (np.isfinite(np.float32(radius)) and np.float32(radius) > 0):
        raise ValueError(f"denoise radius must be finite and > 0, got {parts[0]!r}")
    if min_neighbors < 0 or min_neighbors != parts[1]:
        raise ValueError(f"denoise min_neighbors must be an integer >= 0, got {parts[1]!r}")
    if min_days < 1 or (len(parts) == 3 and min_days != parts[2]):
        raise ValueError(f"denoise min_days must be an integer >= 1, got {parts[2]!r}")
    if min_days > 1 and not days_allowed:
        raise ValueError("kmeans_assign filters a day by its own counts: denoise takes (radius, min_neighbors) there")
    return radius, min_neighbors, min_days


def _denoise_clouds(clouds, denoise, support: Optional[Callable], by_cloud: bool):
    """Drop the rows without support from the union of ``clouds`` (group = cloud index when
    ``by_cloud``, else one group) -> (the clouds with only the kept rows -- a cloud may come out
    empty --, the ``denoise`` result dict)."""
    radius, min_neighbors, min_days = _denoise_args(denoise, by_cloud)
    G = len(clouds) if by_cloud else 1
    if min_days > 1 and G > 64:
        raise ValueError(f"denoise with min_days > 1 takes at most 64 clouds (groups), got {G}")
    sizes = [c.shape[0] for c in clouds]
    X = np.concatenate(clouds).astype(np.float32)          # boundary cast
    groups = np.repeat(np.arange(len(clouds)), sizes) if by_cloud else np.zeros(X.shape[0], dtype=np.int64)
    kept = np.asarray((support or _gpu_support)(X, groups, G, radius, min_neighbors, min_days)).astype(bool)
    if kept.shape != (X.shape[0],):
        raise ValueError("support must return one bool per row")
    if not kept.any():
        raise ValueError(f"denoise removed every point (radius {radius}, min_neighbors {min_neighbors}, "
                         f"min_days {min_days})")
    out, removed, at = [], [], 0
    for c, m in zip(clouds, sizes):
        k = kept[at:at + m]
        out.append(c[k])
        removed.append(int(m - k.sum()))
        at += m
    return out, dict(kept=kept, radius=radius, min_neighbors=min_neighbors, min_days=min_days, removed=removed)


def _gpu_voxels(X: np.ndarray, size):
    """Host (n, 3) float32 rows -> (centroid per occupied voxel float32 (M, 3), counts (M,), inverse (n,)):
    ``voxel_downsample`` in centroid mode on the origin-0 lattice."""
    import torch

    from .voxel import voxel_downsample

    with _gpu_lock:
        ds = voxel_downsample(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda(), size)
        return ds.points.cpu().numpy(), ds.voxels.counts.cpu().numpy(), ds.voxels.inverse.cpu().numpy()


def _voxel_args(voxel):
    """A size or (vz, vy, vx) -> three positive finite float32 sizes as floats, checked."""
    try:
        with np.errstate(over="ignore"):
            v = np.asarray(voxel, dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError):
        v = np.zeros(0, dtype=np.float32)
    if v.shape == ():
        v = np.full(3, v, dtype=np.float32)
    if v.shape != (3,) or not (np.isfinite(v).all() and (v > 0).all()):
        raise ValueError(f"voxel must be None, a size or (vz, vy, vx), finite and > 0 in float32, got {voxel!r}")
    return tuple(float(t) for t in v)


def _thin_clouds(clouds, size, voxels: Optional[Callable]):
    """Thin every cloud separately on the common origin-0 lattice (centroid mode) -> (the thinned
    clouds -- they stay distinguishable --, the ``voxel`` result dict)."""
    out, kept_rows, counts, inverse, at = [], [], [], [], 0
    for c in clouds:
        n = c.shape[0]
        pts, cnt, inv = (np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32)) if not n else \
            (voxels or _gpu_voxels)(c.astype(np.float32), size)       # boundary cast
        pts, cnt, inv = np.asarray(pts), np.asarray(cnt), np.asarray(inv).astype(np.int64)
        m = pts.shape[0]
        if pts.shape != (m, 3) or cnt.shape != (m,) or inv.shape != (n,) or (n and not -1 <= inv.min() <= inv.max() < m):
            raise ValueError("voxels must return (points (M, 3), counts (M,), inverse (n,) in [-1, M))")
        out.append(pts.astype(np.float64))
        kept_rows.append(int(m))
        counts.append(cnt.astype(np.int32))
        inverse.append(np.where(inv >= 0, inv + at, -1))
        at += m
    if not at:
        raise ValueError(f"voxel thinning left no point (voxel {size})")
    return out, dict(size=size, kept_rows=kept_rows, counts=np.concatenate(counts), inverse=np.concatenate(inverse))


def kmeans_fuse(clouds: Sequence[np.ndarray], n_clusters: int = 1024, max_iter: int = 300, tol: float = 1e-4,
                seed: int = 1, fit: Optional[Callable] = None, init: str = "rows", device_clouds=None,
                export_path=None, describe: bool = False, stats: Optional[Callable] = None,
                height_map: bool = False, height_map_cell_log2: int = 0, grid: Optional[Callable] = None,
                register: Optional[str] = None, register_to: int = 0, register_max_dist: Optional[float] = None,
                align: Optional[Callable] = None, denoise=None, support: Optional[Callable] = None, voxel=None,
                voxels: Optional[Callable] = None):
    """Fuse per-pair (M_i, 3) z,y,x clouds into one K-means reconstruction.

    Returns (layers, result) where ``result`` has labels (N,), centers (K, 3),
    inertia, n_iter.  ``init``: ``"rows"`` = rows ``sorted(default_rng(seed).choice(N, K))``
    (SURVEY.md §8d); ``"k-means++"`` = GPU k-means++ with ``random_state=seed``
    (scikit-learn's KMeans default, sklearn/cluster/_kmeans.py:1012-1019).
    K is clipped to N.  ``device_clouds``: the same clouds already on the GPU
    (the plugin's GPU assembly) -- the K-means reads them there.  ``export_path``:
    also write the fused cloud (``export_fused``).

    ``describe=True`` adds one exact statistics pass over the labelled cloud
    (``cluster_stats``; the group of a point is the index of its cloud among the
    non-empty ``clouds``, at most 256): the centroid layer gains ``roughness``
    (spread along the element's normal, NaN below 3 points), ``normal_z`` (the z
    component of the unit normal, >= 0), ``days_seen`` (clouds with a point on the
    element) and ``height_spread`` (max - min over those clouds of the cloud's
    mean z on the element, 0 with fewer than two); ``result`` gains ``stats`` =
    dict(words (G, K, 16) int64, q, sizes).  ``stats`` lets tests substitute
    (X, labels, groups, k, G) -> words.

    ``height_map=True`` adds one exact raster pass over the labelled cloud
    (``height_grid``; group = cloud index, at most 256; origin (0, 0), cells of
    2^``height_map_cell_log2`` pixels, the shape reaching the largest y and x) and
    appends four image layers and a labels layer, all with ``scale`` (2^s, 2^s):
    "Fused Height Map" (mean z of all clouds per pixel, NaN where empty), "Fused
    Height Spread" (max - min over the clouds of each cloud's mean z, 0 with fewer
    than two), "Fused Coverage" (clouds seen in the pixel), "Fused Surface Height"
    (the z of the centre whose point is the highest in the pixel: the model's
    surface) and "Fused Surface Elements" (that centre's index + 1, 0 = background);
    ``result`` gains ``height_map`` = dict(words (G, 4, H, W) int64, q, cell_log2,
    origin, shape, outside, sizes).  Raises ValueError naming
    ``height_map_cell_log2`` when the words would exceed 4 GiB.  ``grid`` lets tests
    substitute (X, labels, groups, k, G, shape, cell_log2, q) -> (words, outside).

    ``register`` (``"z"``, ``"translation"`` or ``"rigid"``; None: off, every output as
    without it) first puts the clouds into one frame -- every pair's cloud comes in that
    pair's own: the model is fitted on cloud ``register_to`` (an index among the non-empty
    clouds) alone, every other cloud is registered onto its centres (``register_days``,
    group = cloud, at most 256; ``register_max_dist`` trims, off by default) and
    transformed; the fuse above then runs unchanged on the registered points, which the
    fused layer, ``describe`` and ``height_map`` all see.  ``result`` gains
    ``registration``: R (G, 3, 3), t (G, 3), ok, n_iter, converged, inliers, outliers,
    rms_before, rms_after, transforms (G, 12) as NumPy arrays (cloud ``register_to``
    keeps the identity).  ``align`` lets tests substitute
    (X, centers, groups, G, kind, max_dist) -> (registration dict, registered X).

    ``denoise`` (``(radius, min_neighbors)`` or ``(radius, min_neighbors, min_days)``; None:
    off, every output as without it) removes what is not surface, after ``register`` and before
    the fuse: one ``filter_outliers`` pass over the union of the clouds (group = cloud index)
    keeps a row with at least ``min_neighbors`` other rows within ``radius`` and, with
    ``min_days`` > 1 (at most 64 clouds), points of at least that many clouds among itself and
    them.  Every layer, ``describe`` and ``height_map`` see only the kept rows (a cloud may come
    out empty).  ``result`` gains ``denoise``: kept (bool over the concatenated input rows),
    radius, min_neighbors, min_days, removed (per cloud).  ``support`` lets tests substitute
    (X, groups, G, radius, min_neighbors, min_days) -> mask.

    ``voxel`` (a size or ``(vz, vy, vx)``; None: off, every output as without it) thins the clouds
    after ``register`` and ``denoise`` and before the fit: every cloud SEPARATELY is reduced to the
    exact centroids of its occupied voxels (``voxel_downsample``, centroid mode) on the common
    lattice anchored at the origin, so the fit weighs surface, not sampling density, and the clouds
    stay distinguishable: every layer, ``describe``, ``height_map`` and their ``sizes`` see the
    thinned rows.  ``result`` gains ``voxel``: size (vz, vy, vx), kept_rows (per cloud), counts
    (rows per kept voxel, concatenated) and inverse (over the concatenated rows that entered the
    thinning: the thinned row of each, -1 for a NaN or Inf row), so ``labels[inverse]`` labels the
    original points.  ``voxels`` lets tests substitute (X, (vz, vy, vx)) -> (points, counts, inverse).
    """
    clouds = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds if np.asarray(c).size]
    if not clouds:
        raise ValueError("no point cloud layers to fuse")
    voxel_size = None if voxel is None else _voxel_args(voxel)     # a bad voxel= fails before anything is fitted
    if denoise is not None:
        # a bad denoise= fails before anything is fitted
        if _denoise_args(denoise, True)[2] > 1 and len(clouds) > 64:
            raise ValueError(f"denoise with min_days > 1 takes at most 64 clouds (groups), got {len(clouds)}")
    registration = None
    if register is not None:
        if not 0 <= int(register_to) < len(clouds):
            raise ValueError(f"register_to must index one of the {len(clouds)} non-empty clouds, got {register_to}")
        ref = int(register_to)
        ref_dev = None if device_clouds is None else [[c for c in device_clouds if c.numel()][ref]]
        _, model = kmeans_fuse([clouds[ref]], n_clusters, max_iter, tol, seed=seed, fit=fit, init=init,
                               device_clouds=ref_dev)
        clouds, registration = _register_clouds(clouds, model["centers"], ref, register, register_max_dist, align)
        device_clouds = None       # the registered rows are on the host
    denoised = None
    if denoise is not None:
        clouds, denoised = _denoise_clouds(clouds, denoise, support, True)
        device_clouds = None       # the kept rows are on the host
    thinned = None
    if voxel_size is not None:
        clouds, thinned = _thin_clouds(clouds, voxel_size, voxels)
        device_clouds = None       # the centroids are on the host
    if describe and len(clouds) > 256:
        raise ValueError(f"describe=True takes at most 256 clouds (groups), got {len(clouds)}")
    if height_map and len(clouds) > 256:
        raise ValueError(f"height_map=True takes at most 256 clouds (groups), got {len(clouds)}")
    X = np.concatenate(clouds).astype(np.float32)          # boundary cast
    Xfit = X
    if device_clouds is not None and fit is None:
        import torch
        Xfit = torch.cat([c.reshape(-1, 3) for c in device_clouds if c.numel()]).to(torch.float32)   # same rounding
    n = X.shape[0]
    k = int(min(n_clusters, n))
    if init == "k-means++":
        C0 = _gpu_kpp(Xfit, k, seed)
    elif init == "rows":
        C0 = X[np.sort(np.random.default_rng(seed).choice(n, k, replace=False))]
    else:
        raise ValueError(f"init must be 'rows' or 'k-means++', got {init!r}")
    labels, centers, inertia, n_iter = (fit or _gpu_fit)(Xfit, C0, int(max_iter), _tolerance(X, tol))
    counts = np.bincount(labels, minlength=k)
    cprops = {"height": _norm(centers[:, 0].astype(np.float64)), "count": counts}
    st = None
    if describe:
        from .stats import surface_elements
        sizes = [c.shape[0] for c in clouds]
        st = _describe(X, labels, sizes, k, Xfit if (stats is None and Xfit is not X) else X, stats)
        se = surface_elements(st)
        present = st.counts() > 0                                   # (G, K)
        mz = np.where(present, st.means()[..., 0], np.nan)
        with np.errstate(invalid="ignore"):
            spread = np.where(present.sum(0) >= 2, np.fmax.reduce(mz, axis=0) - np.fmin.reduce(mz, axis=0), 0.0)
        cprops.update(roughness=se.roughness, normal_z=se.normal[:, 0], days_seen=present.sum(0).astype(np.int64),
                      height_spread=np.nan_to_num(spread, nan=0.0))
    layers = [
        (centers.astype(np.float64),
         {"name": f"{PREFIX} Fused K-means Centroids", "size": 4,
          "properties": cprops,
          "scale": (1, 1, 1), "opacity": 1.0, "face_colormap": "turbo", "face_color": "height"},
         "points"),
        (X.astype(np.float64),
         {"name": f"{PREFIX} Fused {CLOUD_LAYER_SUFFIX}", "size": 2,
          "properties": {"cluster": labels.astype(np.int32), "height": _norm(X[:, 0].astype(np.float64))},
          "scale": (1, 1, 1), "opacity": 0.8, "face_colormap": "turbo", "face_color": "cluster"},
         "points"),
    ]
    result = dict(labels=labels, centers=centers, inertia=inertia, n_iter=n_iter, n_points=n)
    if st is not None:
        result["stats"] = dict(words=st.numpy(), q=list(st.q), sizes=sizes)
    if height_map:
        more, result["height_map"] = _height_map(X, labels, centers, [c.shape[0] for c in clouds], k,
                                                 height_map_cell_log2,
                                                 Xfit if (grid is None and Xfit is not X) else X, grid)
        layers += more
    if registration is not None:
        result["registration"] = registration
    if denoised is not None:
        result["denoise"] = denoised
    if thinned is not None:
        result["voxel"] = thinned
    if export_path is not None:
        export_fused(export_path, X.astype(np.float64), result)
    return layers, result


def _gpu_assign(X, C: np.ndarray):
    """X: host (N, 3) float32 array, or the cloud already on the device -> (labels, squared distances, inertia)."""
    import torch

    from .predict import lloyd_predict

    with _gpu_lock:
        Xt = X.to(torch.float32).contiguous() if isinstance(X, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
        res = lloyd_predict(Xt, torch.from_numpy(np.ascontiguousarray(C, dtype=np.float32)).cuda(),
                            return_distance=True, return_inertia=True)
        torch.cuda.synchronize()
        return res.labels.cpu().numpy(), res.distance.cpu().numpy(), float(res.inertia)


def _gpu_nearest(X: np.ndarray, Y: np.ndarray, max_dist: float):
    """Host (n, 3) and (m, 3) float32 rows -> (index int32 (n,), squared distance float32 (n,)) of
    ``nearest_points``: the nearest row of ``Y`` within ``max_dist``, -1 / +inf when there is none."""
    import torch

    from .nearest import nearest_points

    with _gpu_lock:
        near = nearest_points(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda(),
                              torch.from_numpy(np.ascontiguousarray(Y, dtype=np.float32)).cuda(), max_dist)
        return near.index.cpu().numpy(), near.sqdist.cpu().numpy()


def _change_args(change, change_to, model, name: str = "change"):
    """``change=max_dist`` (or ``change_plane=radius``) and its reference points -> (the distance as a float, the
    reference rows float32 (M, 3)), checked."""
    try:
        with np.errstate(over="ignore", under="ignore"):
            r = np.float32(change)
            r2 = np.float32(r * r)
    except (TypeError, ValueError):
        r = r2 = np.float32(np.nan)
    if not (np.isfinite(r) and r > 0 and np.isfinite(r2) and r2 > 0):
        raise ValueError(f"{name} must be None or a {'max_dist' if name == 'change' else 'radius'} finite and > 0 in "
                         f"float32 (and its square), got {change!r}")
    ref = change_to
    if ref is None and isinstance(model, dict):
        ref = model.get("points")
    if ref is None:
        raise ValueError(f"{name}= needs reference points: pass change_to= (an (M, 3) array or a list of clouds, "
                         "z, y, x) or a model that carries its points (export_fused / load_fused)")
    if isinstance(ref, (list, tuple)):
        parts = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in ref if np.asarray(c).size]
        ref = np.concatenate(parts) if parts else np.zeros((0, 3))
    ref = np.asarray(ref, dtype=np.float64)
    if ref.ndim != 2 or ref.shape[1] != 3:
        raise ValueError(f"change_to must be an (M, 3) array or a list of (M_i, 3) clouds, got shape {ref.shape}")
    return float(r), np.ascontiguousarray(ref.astype(np.float32))          # boundary cast


def _change(X: np.ndarray, ref: np.ndarray, max_dist: float, nearest: Optional[Callable]):
    """The cloud-to-cloud distance of the labelled rows ``X`` to ``ref`` -> the ``change`` result dict."""
    index, sq = (nearest or _gpu_nearest)(X, ref, max_dist)
    index = np.asarray(index).astype(np.int32)
    sq = np.asarray(sq, dtype=np.float32)
    if index.shape != (X.shape[0],) or sq.shape != (X.shape[0],) or (index.size and not -1 <= index.min() <= index.max() < max(ref.shape[0], 1)):
        raise ValueError("nearest must return (index (n,) in [-1, M), squared distance (n,))")
    found = index >= 0
    distance = np.where(found, np.sqrt(sq.astype(np.float64)), np.nan)
    dz = np.full(X.shape[0], np.nan)
    dz[found] = X[found, 0].astype(np.float64) - ref[index[found], 0].astype(np.float64)
    return dict(index=index, distance=distance, dz=dz, max_dist=max_dist, found=found)


def _gpu_planes(X: np.ndarray, Y: np.ndarray, radius: float):
    """Host (n, 3) and (m, 3) float32 rows -> (distance float32 (n,), normal float32 (n, 3), count int64 (n,)) of
    ``point_normals(X, radius, targets=Y)``: the plane through the rows of ``Y`` within ``radius`` of each row."""
    import torch

    from .moments import point_normals

    with _gpu_lock:
        pn = point_normals(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda(), radius,
                           targets=torch.from_numpy(np.ascontiguousarray(Y, dtype=np.float32)).cuda())
        return pn.distance.cpu().numpy(), pn.normal.cpu().numpy(), pn.count.cpu().numpy()


def _change_plane(X: np.ndarray, ref: np.ndarray, radius: float, planes: Optional[Callable]):
    """The point-to-plane distance of the labelled rows ``X`` to the local surface of ``ref`` -> the
    ``change_plane`` result dict."""
    distance, normal, count = (planes or _gpu_planes)(X, ref, radius)
    distance, normal = np.asarray(distance, dtype=np.float64), np.asarray(normal, dtype=np.float64)
    count = np.asarray(count).astype(np.int64)
    n = X.shape[0]
    if distance.shape != (n,) or normal.shape != (n, 3) or count.shape != (n,):
        raise ValueError("planes must return (distance (n,), normal (n, 3), count (n,))")
    few = count < 3                                          # no plane through fewer than three points
    return dict(distance=np.where(few, np.nan, distance), normal=np.where(few[:, None], np.nan, normal), count=count,
                radius=radius)


def kmeans_assign(clouds: Sequence[np.ndarray], model, assign: Optional[Callable] = None, device_clouds=None,
                  describe: bool = False, stats: Optional[Callable] = None, register: Optional[str] = None,
                  register_max_dist: Optional[float] = None, align: Optional[Callable] = None, denoise=None,
                  support: Optional[Callable] = None, change=None, change_to=None, nearest: Optional[Callable] = None,
                  change_plane=None, planes: Optional[Callable] = None):
    """Label per-pair (M_i, 3) z,y,x clouds against a fitted model, without refitting.

    ``model``: a ``kmeans_fuse`` result dict, a ``load_fused`` dict, or the path of
    an ``export_fused`` file; its ``centers`` are used as they are.  Returns
    (layers, result): one points layer with the per-point ``cluster`` (int32),
    ``residual`` (Euclidean distance to the assigned centre, float64: a per-point
    change measure against the model) and ``height``; ``result`` has labels,
    distance (= residual), inertia, n_points.  Same boundary cast (float64 ->
    float32) and ``device_clouds`` shortcut as ``kmeans_fuse``; ``assign`` lets
    tests substitute (X, C) -> (labels, squared distances, inertia).

    ``describe=True`` appends a second points layer ``"... Surface Change"``: the
    model's centres with ``count`` (assigned points), ``dz`` (mean z of the
    assigned points minus the centre's z, 0 where none) and ``rms`` (rms distance
    of the assigned points to their mean, 0 where none), from one exact
    ``cluster_stats`` pass; ``result`` gains ``stats`` = dict(words (1, K, 16), q,
    sizes).  ``stats``: the test stand-in of ``kmeans_fuse``.

    ``register`` (as in ``kmeans_fuse``) first registers every cloud onto the model's
    centres and labels the registered points: ``dz`` and ``residual`` then measure change,
    not the frames' offset.  ``result`` gains ``registration``; ``align``: the test stand-in.

    ``denoise`` = ``(radius, min_neighbors)`` first drops the rows of the (registered) clouds
    with fewer than ``min_neighbors`` other rows within ``radius`` -- the later day is filtered
    by its own counts, as one group; a ``min_days`` above 1 raises ValueError -- and labels the
    rest.  ``result`` gains ``denoise`` as in ``kmeans_fuse``; ``support``: the test stand-in.

    ``change`` = ``max_dist`` adds the cloud-to-cloud distance (``nearest_points``): for every
    labelled row -- after ``register`` and ``denoise`` -- the nearest reference point within
    ``max_dist``.  The reference points are ``change_to`` (an (M, 3) array or a list of clouds, z, y,
    x) or, without it, the model's ``points`` (an ``export_fused`` / ``load_fused`` model carries
    them); ValueError when neither exists.  The "Assigned" layer gains ``change`` (float64 distance
    to that point, NaN beyond ``max_dist``) and ``change_dz`` (the row's z minus that point's z, NaN
    likewise); ``result`` gains ``change`` = dict(index, distance, dz, max_dist, found).
    ``nearest``: the test stand-in (X, Y, max_dist) -> (index, squared distance).

    ``change_plane`` = ``radius`` adds the change along the surface normal (``point_normals``): for
    every labelled row -- after ``register`` and ``denoise`` -- the plane through the reference points
    within ``radius`` of it.  On a sloped surface the distance to the nearest reference POINT is
    dominated by sampling; the distance to that plane is not.  With or without ``change``; the
    reference points follow ``change``'s rule (``change_to``, else the model's ``points``, else
    ValueError).  The "Assigned" layer gains ``change_normal`` (float64: the signed point-to-plane
    distance, positive above the reference surface, NaN where fewer than 3 reference points lie within
    ``radius``) and ``change_normal_z`` (the plane normal's z, NaN likewise); ``result`` gains
    ``change_plane`` = dict(distance, normal, count, radius).  ``planes``: the test stand-in
    (X, ref, radius) -> (distance, normal, count).
    """
    if not isinstance(model, dict):
        model = load_fused(model)
    C = np.ascontiguousarray(np.asarray(model["centers"], dtype=np.float64).astype(np.float32))
    if C.ndim != 2 or C.shape[1] != 3 or C.shape[0] < 1:
        raise ValueError("model centers must be (K, 3)")
    clouds = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds if np.asarray(c).size]
    if not clouds:
        raise ValueError("no point cloud layers to assign")
    if denoise is not None:
        _denoise_args(denoise, False)
    if change is not None:
        # a bad change= fails before anything is labelled
        change_dist, change_ref = _change_args(change, change_to, model)
    if change_plane is not None:
        plane_radius, plane_ref = _change_args(change_plane, change_to, model, "change_plane")
    registration = None
    if register is not None:
        clouds, registration = _register_clouds(clouds, C, None, register, register_max_dist, align)
        device_clouds = None       # the registered rows are on the host
    denoised = None
    if denoise is not None:
        clouds, denoised = _denoise_clouds(clouds, denoise, support, False)
        device_clouds = None       # the kept rows are on the host
    X = np.concatenate(clouds).astype(np.float32)          # boundary cast
    Xq = X
    if device_clouds is not None and assign is None:
        import torch
        Xq = torch.cat([c.reshape(-1, 3) for c in device_clouds if c.numel()]).to(torch.float32)   # same rounding
    labels, sq, inertia = (assign or _gpu_assign)(Xq, C)
    labels = np.asarray(labels).astype(np.int32)
    residual = np.sqrt(np.asarray(sq, dtype=np.float64))
    props = {"cluster": labels, "residual": residual, "height": _norm(X[:, 0].astype(np.float64))}
    changed = None
    if change is not None:
        changed = _change(X, change_ref, change_dist, nearest)
        props.update(change=changed["distance"], change_dz=changed["dz"])
    plane = None
    if change_plane is not None:
        plane = _change_plane(X, plane_ref, plane_radius, planes)
        props.update(change_normal=plane["distance"], change_normal_z=plane["normal"][:, 0])
    layers = [
        (X.astype(np.float64),
         {"name": f"{PREFIX} Assigned {CLOUD_LAYER_SUFFIX}", "size": 2,
          "properties": props,
          "scale": (1, 1, 1), "opacity": 0.8, "face_colormap": "turbo", "face_color": "cluster"},
         "points"),
    ]
    result = dict(labels=labels, distance=residual, inertia=float(inertia), n_points=X.shape[0])
    if registration is not None:
        result["registration"] = registration
    if denoised is not None:
        result["denoise"] = denoised
    if changed is not None:
        result["change"] = changed
    if plane is not None:
        result["change_plane"] = plane
    if describe:
        k = C.shape[0]
        st = _describe(X, labels, [X.shape[0]], k, Xq if (stats is None and Xq is not X) else X, stats)
        cnt = st.counts()[0]
        dz = np.nan_to_num(st.offsets(C)[0, :, 0], nan=0.0)                                        # NaN: no point
        rms = np.nan_to_num(np.sqrt(np.maximum(np.trace(st.covariances()[0], axis1=1, axis2=2), 0.0)), nan=0.0)
        layers.append(
            (C.astype(np.float64),
             {"name": f"{PREFIX} Surface Change", "size": 4,
              "properties": {"count": cnt, "dz": dz, "rms": rms},
              "scale": (1, 1, 1), "opacity": 1.0, "face_colormap": "turbo", "face_color": "dz"},
             "points"))
        result["stats"] = dict(words=st.numpy(), q=list(st.q), sizes=[X.shape[0]])
    return layers, result


class HeightMapExtractor(SatellitePlugin):
    """Multi-day 3D point clouds from WV3 stereo pairs, fused by GPU K-means."""

    requires_image = False

    def __init__(self, base=None, n_clusters: int = 1024, max_iter: int = 300, tol: float = 1e-4,
                 fit: Optional[Callable] = None, init: str = "rows", seed: int = 1, stages=None,
                 export_path=None, _assemble: Optional[Callable] = None, model=None,
                 assign: Optional[Callable] = None, describe: bool = False, stats: Optional[Callable] = None,
                 height_map: bool = False, height_map_cell_log2: int = 0, grid: Optional[Callable] = None,
                 register: Optional[str] = None, register_to: int = 0, register_max_dist: Optional[float] = None,
                 align: Optional[Callable] = None, denoise=None, support: Optional[Callable] = None, voxel=None,
                 voxels: Optional[Callable] = None, change=None, change_to=None, nearest: Optional[Callable] = None,
                 change_plane=None, planes: Optional[Callable] = None):
        self._base = base
        # change_plane: add the point-to-plane distance to the assigned layer (kmeans_assign change_plane=); planes: test stand-in
        self.change_plane = change_plane
        self._planes = planes
        # change: add the cloud-to-cloud distance to the assigned layer (kmeans_assign change=); nearest: test stand-in
        self.change = change
        self.change_to = change_to
        self._nearest = nearest
        # voxel: thin every cloud onto a lattice before the fit (kmeans_fuse voxel=); voxels: test stand-in
        self.voxel = voxel
        self._voxels = voxels
        # denoise: drop the rows without support first (kmeans_fuse / kmeans_assign denoise=); support: test stand-in
        self.denoise = denoise
        self._support = support
        # register: co-register the run's clouds first (kmeans_fuse / kmeans_assign register=); align: test stand-in
        self.register = register
        self.register_to = register_to
        self.register_max_dist = register_max_dist
        self._align = align
        # model: a fitted model (kmeans_fuse result, load_fused dict or export_fused path); when given,
        # run fuses nothing and labels the run's clouds against it (kmeans_assign)
        self.model = model
        self._assign = assign
        # describe: add the per-element statistics (kmeans_fuse / kmeans_assign describe=True); stats: test stand-in
        self.describe = describe
        self._stats = stats
        # height_map: append the fused raster layers (kmeans_fuse height_map=True); grid: test stand-in
        self.height_map = height_map
        self.height_map_cell_log2 = height_map_cell_log2
        self._grid = grid
        self._stages = stages
        self.export_path = export_path
        self._assemble = _assemble   # tests: a CPU stand-in for the GPU assembly (disparity, validity) -> (pts, h_norm)
        self.init = init
        self.seed = seed
        self.n_clusters = n_clusters
        self.max_iter = max_iter
        self.tol = tol
        self._fit = fit
        self.last_result = None

    @property
    def name(self):
        return "Multi-day 3D Point Cloud"

    def _gpu_stages_run(self, stages, kml_path, is_debug_mode, is_debug_pair, is_one_random_pair, n) -> List:
        from .pipeline import pair_layers
        layers, host_clouds, dev_clouds = [], [], []
        for pp in stages.pairs(kml_path, is_debug_mode=is_debug_mode, is_debug_pair=is_debug_pair,
                               is_one_random_pair=is_one_random_pair, n=n):
            layers += list(pp.image_layers)
            if self._assemble is not None:
                pts, hn = self._assemble(pp.disparity, pp.validity)
                dev = None
            else:
                from .cloud import assemble_cloud_device
                with _gpu_lock:
                    dev, hn_d, _ = assemble_cloud_device(pp.disparity, pp.validity)
                    pts, hn = dev.cpu().numpy(), hn_d.cpu().numpy()
            layers += pair_layers(pp, pts, hn)
            host_clouds.append(pts)
            dev_clouds.append(dev)
        if not host_clouds:
            return layers
        if self.model is not None:
            use_dev = self._assign is None and all(d is not None for d in dev_clouds)
            assigned, self.last_result = kmeans_assign(host_clouds, self.model, assign=self._assign,
                                                       device_clouds=dev_clouds if use_dev else None,
                                                       describe=self.describe, stats=self._stats,
                                                       register=self.register,
                                                       register_max_dist=self.register_max_dist, align=self._align,
                                              denoise=self.denoise, support=self._support,
                                                       change=self.change, change_to=self.change_to,
                                                       nearest=self._nearest, change_plane=self.change_plane,
                                                       planes=self._planes)
            return layers + assigned
        use_dev = self._fit is None and all(d is not None for d in dev_clouds)
        fused, self.last_result = kmeans_fuse(host_clouds, self.n_clusters, self.max_iter, self.tol, seed=self.seed,
                                              fit=self._fit, init=self.init,
                                              device_clouds=dev_clouds if use_dev else None,
                                              export_path=self.export_path, describe=self.describe,
                                              stats=self._stats, height_map=self.height_map,
                                              height_map_cell_log2=self.height_map_cell_log2, grid=self._grid,
                                              register=self.register, register_to=self.register_to,
                                              register_max_dist=self.register_max_dist, align=self._align,
                                              denoise=self.denoise, support=self._support, voxel=self.voxel,
                                              voxels=self._voxels)
        return layers + fused

    def _stages_run(self, kml_path, is_debug_mode, is_debug_pair, is_one_random_pair, n) -> List:
        from .pipeline import CropFailed, ImageNotFound, ReferenceStereoStages
        stages = self._stages or ReferenceStereoStages()
        log = getattr(stages, "log", lambda msg: None)
        try:
            layers = self._gpu_stages_run(stages, kml_path, is_debug_mode, is_debug_pair, is_one_random_pair, n)
            log(f"Added {len(layers)} layers to Napari")
            return layers
        except ImageNotFound:                      # plugin.py:77-79
            return [(np.zeros((100, 100)), {"name": "error: image not found"}, "image")]
        except CropFailed as e:                    # plugin.py:89-91
            return [(np.zeros((100, 100)), {"name": f"error: {str(e)}"}, "image")]
        except Exception as e:                     # plugin.py:236-241
            import traceback
            traceback.print_exc()
            log(f"Error: {str(e)}\n{traceback.format_exc()}")
            return [(np.ones((100, 100)), {"name": f"Error: {str(e)}"}, "image")]
        finally:
            getattr(stages, "close_log", lambda: None)()

    def run(self, kml_path, is_debug_mode: bool = DEFAULTS["is_debug_mode"],
            is_debug_pair: bool = DEFAULTS["is_debug_pair"],
            is_one_random_pair: bool = DEFAULTS["is_one_random_pair"], n: int = DEFAULTS["n"]) -> List:
        try:
            if self._base is None:
                return self._stages_run(kml_path, is_debug_mode, is_debug_pair, is_one_random_pair, n)
            layers = list(self._base.run(kml_path, is_debug_mode=is_debug_mode, is_debug_pair=is_debug_pair,
                                         is_one_random_pair=is_one_random_pair, n=n))
            clouds = [data for data, params, kind in layers
                      if kind == "points" and str(params.get("name", "")).endswith(CLOUD_LAYER_SUFFIX)]
            if not clouds:   # the pipeline returned only images (or an error layer): pass it through
                return layers
            if self.model is not None:
                assigned, self.last_result = kmeans_assign(clouds, self.model, assign=self._assign,
                                                           describe=self.describe, stats=self._stats,
                                                           register=self.register,
                                                           register_max_dist=self.register_max_dist,
                                                           align=self._align, denoise=self.denoise,
                                                           support=self._support, change=self.change,
                                                           change_to=self.change_to, nearest=self._nearest,
                                                           change_plane=self.change_plane, planes=self._planes)
                return layers + assigned
            fused, self.last_result = kmeans_fuse(clouds, self.n_clusters, self.max_iter, self.tol, seed=self.seed,
                                                  fit=self._fit, init=self.init, export_path=self.export_path,
                                                  describe=self.describe, stats=self._stats,
                                                  height_map=self.height_map,
                                                  height_map_cell_log2=self.height_map_cell_log2, grid=self._grid,
                                                  register=self.register, register_to=self.register_to,
                                                  register_max_dist=self.register_max_dist, align=self._align,
                                                  denoise=self.denoise, support=self._support, voxel=self.voxel,
                                                  voxels=self._voxels)
            return layers + fused
        except Exception as e:   # reference convention: an error layer, never an exception
            import traceback
            traceback.print_exc()
            return [(np.ones((100, 100)), {"name": f"Error: {e}"}, "image")]
