"""Time ``pcm_cluster_stats`` (the exact per-(group, cluster) moments pass) against
the PyTorch route to the same table on the same GPU in the same run:
``table.index_add_(0, g * K + label, [1, x, x (x) x])`` in float64 into a
(G K, 10) table -- not exact (float adds in arrival order), the yardstick only.

Inputs: K = 1024, D = 3 fp32, labels from ``lloyd_predict`` against the centres
of ``--iters`` Lloyd iterations, G = 1 and G = 8 (the rows split into G
contiguous clouds, as the plugin concatenates the days), on

* the raster height-map cloud (14.4M points, the order the plugin delivers);
* the uniform cloud in generation order (14.4M and 100M points): neighbouring
  rows are unrelated, so the lanes of a wave hold different clusters and the rows
  take the straggler path (per-lane atomics).

HIP events on the current stream, warm, median of ``reps`` back-to-back runs.
"kernel" is the buffer clear plus ``pcm_cluster_stats``; "torch" forms the
(n, 10) float64 rows and adds them, "index_add_ alone" adds rows formed
beforehand.  Each line gives the stream floor (17 B per point: 12 B of
coordinates, 4 B label, 1 B group, over 8 TB/s) and the fraction of it reached,
and whether the words of two different grid sizes are bit-equal.
usage: python tools/stats_timing.py [--out FILE] [--reps R] [--iters I] [--small]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcm_amd import _lib, lloyd, lloyd_predict  # noqa: E402
from pcm_amd.engine import Engine, synth_uniform  # noqa: E402
from pcm_amd.stats import accumulate  # noqa: E402
from predict_timing import raster_cloud, timed  # noqa: E402

HBM = 8.0e12     # B/s
BYTES = 17.0     # per point


def torch_rows(X):
    x = X.double()
    iu = torch.triu_indices(3, 3, device=X.device)
    return torch.cat([torch.ones_like(x[:, :1]), x, x[:, iu[0]] * x[:, iu[1]]], dim=1)


def case(name, X, k, reps, iters, lines):
    n, d = X.shape
    C0 = X[torch.from_numpy(np.sort(np.random.default_rng(1).choice(n, k, replace=False))).cuda()].contiguous()
    eng = Engine(d, k, torch.float32, max_iter=max(1, iters))
    q, _ = lloyd.prepare(eng, X, lloyd.LOCAL)
    eng.begin(C0, 0.0, max(1, iters))
    eng.iterate(iters)
    C = eng.centers().clone()
    del eng
    labels = lloyd_predict(X, C).labels
    qa = np.ascontiguousarray(np.asarray(q, dtype=np.int32))
    W = _lib.stats_words(d)
    floor_ms = n * BYTES / HBM * 1e3
    for G in (1, 8):
        g8 = None if G == 1 else (torch.arange(n, device="cuda") * G // n).to(torch.uint8)
        key = labels.long() if G == 1 else g8.long() * k + labels.long()
        buf = torch.empty(G * k * W + 1, dtype=torch.int64, device="cuda")

        def kernel():
            buf.zero_()
            accumulate(X, labels, g8, G, k, qa, buf)
            return buf

        def route():
            return torch.zeros(G * k, 10, dtype=torch.float64, device="cuda").index_add_(0, key, torch_rows(X))

        t_k, _ = timed(kernel, reps)
        words = buf.clone()
        t_r, table = timed(route, reps)
        rows = torch_rows(X)
        t_i, _ = timed(lambda: torch.zeros(G * k, 10, dtype=torch.float64, device="cuda").index_add_(0, key, rows), reps)
        del rows
        # the words do not depend on the grid
        os.environ["PCM_STATS_BLOCKS"] = "97"
        kernel()
        equal = bool(torch.equal(buf, words))
        del os.environ["PCM_STATS_BLOCKS"]
        # and agree with the float table to its rounding: counts exactly, first moments to 1e-9
        w = words[:-1].view(G * k, W)
        counts_ok = bool(torch.equal(w[:, 0], table[:, 0].long()))
        scale = torch.tensor([2.0 ** -int(v) for v in qa], dtype=torch.float64, device="cuda")
        # (the table sums x, the words sum trunc(x 2^q): they differ by the truncation, below n 2^-q per cluster)
        dev = float(((w[:, 1:1 + d].double() * scale - table[:, 1:1 + d]).abs() / (w[:, :1].double() + 1) / scale).max())
        lines.append(f"{name} n={n} k={k} d={d} fp32 G={G}: kernel {t_k:.3f} ms ({floor_ms / t_k * 100:.1f} % of the "
                     f"{floor_ms:.3f} ms stream floor), torch float64 route {t_r:.3f} ms ({t_r / t_k:.1f}x), "
                     f"index_add_ alone {t_i:.3f} ms ({t_i / t_k:.1f}x); skipped {int(words[-1])}; grids bit-equal: "
                     f"{equal}; counts equal torch's: {counts_ok}; mean truncation per row {dev:.2f} ulp of 2^-q")
        print(lines[-1], flush=True)
        del table, key, g8, buf, words
    del labels
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="14.4M-point inputs only")
    a = ap.parse_args()
    k, d = 1024, 3
    lines = [f"# tools/stats_timing.py: {torch.cuda.get_device_name(0)}, HIP events, warm, median of {a.reps}; "
             f"labels of lloyd_predict against the centres after {a.iters} Lloyd iterations"]
    case("raster height-map cloud", raster_cloud(int(round(14_400_000 ** 0.5))), k, a.reps, a.iters, lines)
    for n in (14_400_000,) if a.small else (14_400_000, 100_000_000):
        case("uniform cloud (generation order)", synth_uniform(n, d, seed=0), k, a.reps, a.iters, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
