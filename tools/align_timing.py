"""Time the registration pass ``pcm_align_stats`` (k_align) and a whole ``register_days`` run against
the route composed from the rest of the API on the same GPU in the same run: a torch transform
(``X[day] @ R.T + t`` on each day's contiguous rows), ``lloyd_predict`` and ``cluster_stats`` -- the sums of the points per
(day, centre), from which the same solve could be formed -- with ``max_dist=None``.

Inputs: K = 1024 centres of ``--iters`` Lloyd iterations, D = 3 fp32, the rows split into G = 4
contiguous days (as the plugin concatenates them), each day displaced by a small rigid motion, on

* the raster height-map cloud (14.4M points, the order the plugin delivers);
* the uniform cloud in generation order (14.4M points): neighbouring rows are unrelated, so the
  lanes of a wave scan different cells' lists.

HIP events on the current stream, warm, median of ``reps`` back-to-back runs.  "k_align" is the
buffer clear plus one ``pcm_align_stats`` on prepared lists (no host synchronisation inside);
"prepare" is the list build with its host copy of the centres; the stream floor is 13 B per point
(12 B of coordinates, 1 B group) over 8 TB/s.  The 187 MB of either input fit the 256 MB Infinity
Cache and the runs are back to back, so these small clouds run warm in it, as the predict rows
do: the HBM floor is a reference line, not the bound that applies.  ``register_days`` is wall
clock and includes the host solves and one synchronisation per iteration.  No speed threshold is
asserted anywhere: this file records.
usage: python tools/align_timing.py [--out FILE] [--reps R] [--iters I]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcm_amd import align, cluster_stats, lloyd, lloyd_predict  # noqa: E402
from pcm_amd.engine import Engine, synth_uniform  # noqa: E402
from predict_timing import raster_cloud, timed  # noqa: E402

HBM = 8.0e12     # B/s
BYTES = 13.0     # per point
G = 4


def motions(rng):
    T = np.zeros((G, 12))
    for g in range(G):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        th = np.deg2rad(0.02) * g
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        T[g, :9] = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)).ravel()
    return T.astype(np.float32)


def case(name, X, k, reps, iters, lines):
    n, d = X.shape
    C0 = X[torch.from_numpy(np.sort(np.random.default_rng(1).choice(n, k, replace=False))).cuda()].contiguous()
    eng = Engine(d, k, torch.float32, max_iter=max(1, iters))
    lloyd.prepare(eng, X, lloyd.LOCAL)
    eng.begin(C0, 0.0, max(1, iters))
    eng.iterate(iters)
    C = eng.centers().clone()
    del eng
    g8 = (torch.arange(n, device="cuda") * G // n).to(torch.uint8)
    T = motions(np.random.default_rng(2))
    # every day but the first arrives displaced: a rotation of 0.02 degrees and 1e-3 of the extent per day index
    ext = float((X.amax(0) - X.amin(0)).max())
    T[:, 9:] = np.random.default_rng(3).uniform(-1, 1, (G, 3)) * 1e-3 * ext * np.arange(G)[:, None]
    floor_ms = n * BYTES / HBM * 1e3
    t_p, plan = timed(lambda: align.AlignPlan(C, n, None), reps)
    q = align.default_q(X.abs().amax(0).double().cpu().numpy(), plan.cabs, T)
    st = align.align_stats(X, C, groups=g8, n_groups=G, transforms=T, q=q, plan=plan)

    Td = torch.from_numpy(T).cuda()
    qa = np.ascontiguousarray(np.asarray(q, dtype=np.int32))

    def kernel():
        st._buf.zero_()
        align.accumulate(X, g8, G, Td, float("inf"), qa, st._buf, plan)

    bounds = [(-(-g * n // G), -(-(g + 1) * n // G)) for g in range(G)]     # day g: the rows with i * G // n == g
    assert all(int(g8[a]) == g and int(g8[b - 1]) == g for g, (a, b) in enumerate(bounds))

    def route():
        P = torch.cat([X[a:b] @ Td[g, :9].view(3, 3).T + Td[g, 9:] for g, (a, b) in enumerate(bounds)])
        labels = lloyd_predict(P, C).labels
        return cluster_stats(P, labels, k, groups=g8, n_groups=G)

    t_k, _ = timed(kernel, reps)
    words = st._buf.clone()
    os.environ["PCM_ALIGN_BLOCKS"] = "97"
    kernel()
    equal = bool(torch.equal(st._buf, words))
    del os.environ["PCM_ALIGN_BLOCKS"]
    t_r, _ = timed(route, reps)
    Xm = align.apply_registration(X, T, g8)          # the days as they arrive: displaced
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reg = align.register_days(Xm, C, groups=g8, n_groups=G, kind="rigid", tol=2e-4 * ext)
    torch.cuda.synchronize()
    t_reg = (time.perf_counter() - t0) * 1e3
    lines.append(f"{name} n={n} k={k} G={G} fp32: k_align {t_k:.3f} ms ({floor_ms / t_k * 100:.1f} % of the "
                 f"{floor_ms:.3f} ms stream floor), prepare {t_p:.3f} ms, cells {plan.info['cells']} "
                 f"(FULL {plan.info['full_cells']}); composed route (torch transform + lloyd_predict + cluster_stats) "
                 f"{t_r:.3f} ms ({t_r / t_k:.1f}x); grids bit-equal: {equal}; register_days (rigid, wall clock) "
                 f"{t_reg:.1f} ms for {reg.n_iter} iterations at tol = 2e-4 of the extent, converged {reg.converged}, rms "
                 f"{np.round(reg.rms_before, 4).tolist()} -> {np.round(reg.rms_after, 4).tolist()}")
    print(lines[-1], flush=True)
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    k = 1024
    lines = [f"# tools/align_timing.py: {torch.cuda.get_device_name(0)}, HIP events, warm, median of {a.reps}; "
             f"centres after {a.iters} Lloyd iterations; G = {G} contiguous days"]
    case("raster height-map cloud", raster_cloud(int(round(14_400_000 ** 0.5))), k, a.reps, a.iters, lines)
    case("uniform cloud (generation order)", synth_uniform(14_400_000, 3, seed=0), k, a.reps, a.iters, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
