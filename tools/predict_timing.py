"""Time ``lloyd_predict`` (labels + distances) against the two older routes to
labels for given centres, on the bench's synthetic cloud (counter-based
U[0,1)^3 in generation order: neighbouring rows are unrelated, so the lanes of
a wave fall into different cells -- the unfavourable case for the row-order
kernel), and the 14.4M case again on a raster-ordered height-map cloud, the
order in which the plugin delivers a pair's cloud:

* predict       ``lloyd_predict(X, C, return_distance=True)`` (bounding box, lists, k_predict)
* engine route  ``Engine.bbox + build + begin + final + labels`` (layout sort, E-step, un-permute)
* brute force   ``assign_bruteforce`` without statistics (all K per point)

HIP events on the current stream, warm, median of ``reps`` runs of the same
cloud back to back: a 14.4M-point cloud (172 MB) stays resident in the
Infinity Cache between repetitions, for all three routes alike.  The centres
are those of ``--iters`` Lloyd iterations from the bench's initial rows.
usage: python tools/predict_timing.py [--out FILE] [--reps R] [--iters I] [N K D]...
       (default: 14.4M and 100M points, K = 1024, D = 3)
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcm_amd import lloyd, lloyd_predict  # noqa: E402
from pcm_amd.engine import Engine, assign_bruteforce, synth_rows, synth_uniform  # noqa: E402


def timed(fn, reps):
    fn()                                    # warm: allocator, code objects
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def raster_cloud(side):
    """A per-pair cloud as the plugin assembles it: (z, y, x) of every pixel of a
    side x side height map in raster order (smooth relief + noise, pixel units)."""
    yy, xx = torch.meshgrid(torch.arange(side, device="cuda", dtype=torch.float32),
                            torch.arange(side, device="cuda", dtype=torch.float32), indexing="ij")
    g = torch.Generator(device="cuda").manual_seed(0)
    z = 40 * torch.sin(xx / 230.0) + 25 * torch.cos(yy / 170.0) + torch.randn(xx.shape, device="cuda", generator=g)
    return torch.stack([z, yy, xx], dim=-1).reshape(-1, 3).contiguous()


def case(n, k, d, reps, iters, raster=False):
    if raster:
        X = raster_cloud(int(round(n ** 0.5)))
        n = X.shape[0]
        C0 = X[torch.from_numpy(np.sort(np.random.default_rng(1).choice(n, k, replace=False))).cuda()].contiguous()
    else:
        X = synth_uniform(n, d, seed=0)
        C0 = synth_rows(np.sort(np.random.default_rng(1).choice(n, k, replace=False)), d, seed=0)
    eng = Engine(d, k, torch.float32, max_iter=max(1, iters))
    q, _ = lloyd.prepare(eng, X, lloyd.LOCAL)
    eng.begin(C0, 0.0, max(1, iters))
    eng.iterate(iters)
    C = eng.centers().clone()
    torch.cuda.synchronize()

    def engine_route():
        eng.bbox(X)
        eng.build(X, q, 0)
        eng.begin(C, 0.0, 1)
        eng.final()
        return eng.labels()

    t_pred, res = timed(lambda: lloyd_predict(X, C, return_distance=True), reps)
    t_eng, lab_e = timed(engine_route, reps)
    t_bf, lab_b = timed(lambda: assign_bruteforce(X, C, q), max(1, reps // 2))
    same = bool(torch.equal(res.labels, lab_e)) and bool(torch.equal(res.labels, lab_b))
    return (f"{'raster height-map cloud' if raster else 'uniform cloud'} n={n} k={k} d={d} fp32: "
            f"predict {t_pred:.3f} ms, engine route {t_eng:.3f} ms, brute force {t_bf:.3f} ms; "
            f"predict lists: cells {res.info['cells']}, full {res.info['full_cells']}, mean list "
            f"{res.info['mean_list']:.2f}; labels equal on all three routes: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("shape", nargs="*", type=int)
    a = ap.parse_args()
    shapes = [tuple(a.shape[i:i + 3]) for i in range(0, len(a.shape), 3)] or [(14_400_000, 1024, 3),
                                                                              (100_000_000, 1024, 3)]
    lines = [f"# tools/predict_timing.py: {torch.cuda.get_device_name(0)}, HIP events, warm (back-to-back runs of one "
             f"cloud: 14.4M points stay cache-resident), median of {a.reps} (brute force: {max(1, a.reps // 2)}); centres after {a.iters} Lloyd iterations"]
    for n, k, d in shapes:
        lines.append(case(n, k, d, a.reps, a.iters))
        print(lines[-1], flush=True)
    if not a.shape:   # the 14.4M-point pair cloud again, in the raster order the plugin delivers
        lines.append(case(14_400_000, 1024, 3, a.reps, a.iters, raster=True))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
