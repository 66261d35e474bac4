"""Apply fitted centres to a cloud: labels, distances and inertia without a refit.

``lloyd_predict`` restates the E-step of scikit-learn's ``KMeans.predict`` /
``score`` (``_labels_inertia``, sklearn/cluster/_kmeans.py:1083-1108) in the
canonical float32 arithmetic of the fit's final E-step, through
``pcm_predict``: the cloud is streamed once in the caller's row order against
exact candidate lists of the centres -- no layout sort, no point-sized scratch.
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import _lib
from .engine import _dtype_code, _ptr, _stream
from .fixed import fixed_q, inertia_from_limbs


@dataclass
class LloydPrediction:
    labels: torch.Tensor                    # int32, the caller's row order
    distance: Optional[torch.Tensor]        # float32 canonical SQUARED distance to the assigned centre
    inertia: Optional[float]                # this rank's rows; exact, see ``limbs``
    # pruning facts: cells, full_cells (their points scanned all K centres), list_sum and
    # mean_list over the other cells; all 0 when no lists were built (K = 1)
    info: dict = field(default_factory=dict)
    limbs: Optional[tuple] = None           # (l0, l1, l2, overflow, scale): sum over ranks, then inertia_from_limbs


def predict_q(X: torch.Tensor, centers: torch.Tensor) -> list:
    """Fixed-point exponents over the rows of ``X`` AND ``centers``: the inertia
    scale must bound every distance, and centres may lie outside the cloud."""
    d = centers.shape[1]
    m = centers.abs().amax(0).double()
    if X.shape[0]:
        m = torch.maximum(m, X.abs().amax(0).double())
    m = m.cpu().numpy()
    if not np.isfinite(m).all():
        return [0] * d        # pcm_predict reports the non-finite input
    return fixed_q(m)


def lloyd_predict(X: torch.Tensor, centers: torch.Tensor, *, return_distance: bool = False,
                  return_inertia: bool = False, q=None) -> LloydPrediction:
    """Nearest of ``centers`` (K, D) for every row of ``X`` (n, D), D <= 4,
    float32 or float16, on the device.

    Labels follow the canonical rule (fp32 direct-form distance, strict ``<`` in
    ascending centroid index).  ``q``: the fixed-point exponents the inertia
    scale derives from (default: over ``X`` and ``centers``); multi-rank callers
    pass global exponents and sum ``limbs`` themselves -- every rank predicts its
    own rows, no collective is involved.  Labels and distances never depend on ``q``.
    """
    if not (isinstance(X, torch.Tensor) and X.is_cuda):
        raise _lib.PcmError("lloyd_predict expects a HIP device tensor (no CPU fallback)")
    if X.dim() != 2 or not 1 <= X.shape[1] <= 4:
        raise ValueError("X must be (n, d) with 1 <= d <= 4")
    X = X.contiguous()
    n, d = X.shape
    C = torch.as_tensor(centers).to(device=X.device, dtype=torch.float32).contiguous()
    if C.dim() != 2 or C.shape[1] != d or C.shape[0] < 1:
        raise ValueError(f"centers must be (k, {d}) with k >= 1")
    k = C.shape[0]
    if not torch.isfinite(C).all():
        raise ValueError("centers contain NaN or Inf")
    lib = _lib.load()
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    dist = torch.empty(n, dtype=torch.float32, device=X.device) if return_distance else None
    limbs = _lib.PcmInertia() if return_inertia else None
    qa = None
    if return_inertia:
        qa = np.ascontiguousarray(np.asarray(predict_q(X, C) if q is None else q, dtype=np.int32))
        if qa.shape != (d,):
            raise ValueError(f"q must hold {d} exponents")
    info = (ctypes.c_int64 * 3)()
    nbytes = ctypes.c_size_t()
    _lib.check(lib.pcm_predict_workspace(n, d, k, ctypes.byref(nbytes)), "pcm_predict_workspace")
    ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=X.device)
    rc = lib.pcm_predict(_ptr(X) if n else None, _dtype_code(X), n, d, _ptr(C), k,
                         qa.ctypes.data_as(ctypes.c_void_p) if qa is not None else None,
                         _ptr(labels) if n else None, _ptr(dist) if (dist is not None and n) else None,
                         ctypes.byref(limbs) if limbs is not None else None, info, _ptr(ws), nbytes.value, _stream())
    if rc == -4:
        raise ValueError("input points contain NaN or Inf")
    _lib.check(rc, "pcm_predict")
    cells, full, lsum = int(info[0]), int(info[1]), int(info[2])
    facts = dict(cells=cells, full_cells=full, list_sum=lsum, mean_list=lsum / (cells - full) if cells > full else 0.0)
    inertia, lt = None, None
    if limbs is not None:
        lt = (int(limbs.limbs[0]), int(limbs.limbs[1]), int(limbs.limbs[2]), int(limbs.overflow), int(limbs.scale))
        inertia = inertia_from_limbs(lt[:3], lt[4], lt[3])
    return LloydPrediction(labels=labels, distance=dist, inertia=inertia, info=facts, limbs=lt)
