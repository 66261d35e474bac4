"""Writes recovery_k256.npz: the converged Lloyd centres (oracle.lloyd_ref.lloyd_fit, rows init) of day 0
of the registration tests' terrain (tests/align_ref.py, recovery_days) at K = 256.

    PYTHONPATH=. python tests/golden/align/make_align_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import align_ref as A  # noqa: E402
from oracle import lloyd_ref as R  # noqa: E402

if __name__ == "__main__":
    X0 = A.recovery_days()[0].astype(np.float32)
    fit = R.lloyd_fit(X0, X0[R.init_indices(X0.shape[0], 256)], max_iter=300)
    np.savez(os.path.join(HERE, "recovery_k256.npz"), centers=fit["centers"].astype(np.float32),
             n_iter=np.int64(fit["n_iter"]), n_points=np.int64(X0.shape[0]), strict=np.bool_(fit["strict"]))
    print(fit["n_iter"], fit["strict"], fit["inertia"])
