"""Time ``voxel_grid`` step by step -- ``pcm_voxel_keys``, ``torch.sort`` of the keys,
``pcm_voxel_count`` (heads plus scan), ``pcm_voxel_reduce`` and the call as a whole -- on the same
GPU in the same run as its two yardsticks:

* the PyTorch route on the same keys: ``torch.unique(keys, return_inverse=True, return_counts=True)``
  (its own sort inside) plus a float64 ``index_add_`` of the coordinates -- the accumulate stage;
  that route is not exact (float64 sums in atomic order) and gives neither first rows nor day masks;
* a floor for ``k_voxel_reduce``: the bytes it must move -- per row the sorted key (8), the
  permutation entry (8), the gathered row (12), the group byte (1, with groups) and ``inverse`` (4);
  per voxel ``cells`` (24), ``counts`` (4), ``sums`` (24), ``first`` (4) and the day mask (8, with
  groups) -- at the stream rate recorded in profiles/support_timing.txt (the same GPU model).

Inputs: 14.4M points, fp32: the raster height-map cloud in the order the plugin delivers, and the
uniform cloud in generation order scaled to the same box; three voxel sizes each, chosen for about
1, about 4 and about 30 rows per occupied voxel (the measured mean is printed); without groups and
with G = 4 (the rows split into 4 contiguous clouds).  HIP events on the current stream, warm,
median of ``reps`` back-to-back runs, so every figure here ran WARM: the cloud of 14.4M rows
(173 MB) fits the 256 MB Infinity Cache; sorted keys, permutation and cloud together (403 MB, what
the reduction reads) do not fit it whole.  Every (cloud, size) case runs in a child process of its
own under its own time limit; the first case that fails ends the run.
usage: python tools/voxel_timing.py [--out FILE] [--reps R] [--n N] [--limit SECONDS]
"""
import argparse
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROW_BYTES = 8 + 8 + 12 + 4       # + 1 with groups
VOXEL_BYTES = 24 + 4 + 24 + 4    # + 8 with groups
CASES = {
    "raster": ("raster height-map cloud", ((1.0, 1.0, 1.0), (8.0, 2.0, 2.0), (16.0, 6.0, 5.0))),
    "uniform": ("uniform cloud (generation order)", ((4.0, 2.0, 2.0), (8.0, 6.0, 6.5), (16.0, 12.0, 12.5))),
}


def recorded_stream_rate():
    """The stream rate in B/s that tools/support_timing.py measured and profiles/support_timing.txt records."""
    text = open(os.path.join(ROOT, "profiles", "support_timing.txt")).read()
    return float(re.search(r"stream rate ([0-9.]+) TB/s", text).group(1)) * 1e12


def cloud(kind, n):
    import torch
    from pcm_amd.engine import synth_uniform
    from predict_timing import raster_cloud
    side = int(round(n ** 0.5))
    if kind == "raster":
        return raster_cloud(side)
    scale = torch.tensor([80.0, float(side), float(side)], device="cuda")
    shift = torch.tensor([-40.0, 0.0, 0.0], device="cuda")
    return (synth_uniform(side * side, 3, seed=0) * scale + shift).contiguous()


def one_case(kind, size, n, reps, rate):
    """One (cloud, size): the steps without groups and with G = 4, then the yardstick -> text lines."""
    import torch
    from pcm_amd import _lib, voxel
    from predict_timing import timed
    _lib.load()
    X = cloud(kind, n)
    n = X.shape[0]
    v32, _ = voxel.voxel_sizes(size)
    o32 = np.zeros(3, dtype=np.float32)
    name = CASES[kind][0]
    lines = []
    t_keys, (keys, info) = timed(lambda: voxel.voxel_keys(X, v32, o32), reps)
    t_sort, (skeys, perm) = timed(lambda: torch.sort(keys), reps)
    ws = voxel.workspace(n, X.device)
    t_count, _ = timed(lambda: voxel.voxel_count(skeys, info, ws), reps)
    host = info.tolist()
    assert host[0] == 0, host
    m = int(host[8])
    qa = np.asarray(voxel.fixed_q(np.abs(voxel._decode_box(host[9:15])).reshape(2, 3).max(0).astype(np.float64)), np.int32)
    for G in (1, 4):
        g8 = None if G == 1 else (torch.arange(n, device="cuda") * G // n).to(torch.uint8)
        t_red, out = timed(lambda: voxel.voxel_reduce(X, g8, G, qa, skeys, perm, m, info, ws), reps)
        t_all, vox = timed(lambda: voxel.voxel_grid(X, size, groups=g8, n_groups=G if g8 is not None else None), reps)
        assert torch.equal(vox.counts, out[1]) and torch.equal(vox.sums, out[2]) and torch.equal(vox.inverse, out[5])
        floor_ms = (n * (ROW_BYTES + (G > 1)) + m * (VOXEL_BYTES + 8 * (G > 1))) / rate * 1e3
        lines.append(
            f"{name} n={n} voxel={tuple(float(t) for t in v32)} (M={m}, mean {n / m:.1f} rows per voxel, max "
            f"{int(vox.counts.max())}) G={G}: keys {t_keys:.3f} ms, sort {t_sort:.3f} ms, heads+scan {t_count:.3f} ms, "
            f"reduce {t_red:.3f} ms ({floor_ms / t_red * 100:.1f} % of the {floor_ms:.3f} ms floor: "
            f"{ROW_BYTES + (G > 1)} B per row and {VOXEL_BYTES + 8 * (G > 1)} B per voxel at the recorded "
            f"{rate / 1e12:.2f} TB/s), voxel_grid as a whole {t_all:.3f} ms"
            + ("" if G == 1 else f"; voxels seen by all {G} groups: {int((vox.days() == G).sum())}"))
        del out, vox
    # the yardstick: torch.unique on the same keys, then a float64 index_add_ of the coordinates
    t_uni, (uk, inv, cnt) = timed(lambda: torch.unique(keys, return_inverse=True, return_counts=True), reps)
    X64 = X.double()

    def accumulate():
        return torch.zeros((uk.numel(), 3), dtype=torch.float64, device="cuda").index_add_(0, inv, X64)

    t_acc, acc = timed(accumulate, reps)
    vox = voxel.voxel_grid(X, size)
    same = bool(torch.equal(cnt.to(torch.int32), vox.counts) and torch.equal(inv.to(torch.int32), vox.inverse))
    dev = float(((acc / cnt[:, None]).float() - vox.centroids()).abs().max())
    lines.append(
        f"yardstick, {name} n={n} voxel={tuple(float(t) for t in v32)}: torch.unique(keys, return_inverse, "
        f"return_counts) {t_uni:.3f} ms (pcm: sort + heads+scan {t_sort + t_count:.3f} ms), float64 index_add_ of "
        f"the coordinates {t_acc:.3f} ms (pcm: reduce {t_red:.3f} ms with G=4); counts and inverse equal: {same}; "
        f"largest |float64 centroid - exact centroid| {dev:.3g}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=14_400_000)
    ap.add_argument("--limit", type=int, default=150, help="seconds a (cloud, size) case may take")
    ap.add_argument("--case", default=None, help="internal: KIND:INDEX, run one case in this process")
    a = ap.parse_args()
    rate = recorded_stream_rate()
    if a.case is not None:
        kind, idx = a.case.split(":")
        print("\n".join(one_case(kind, CASES[kind][1][int(idx)], a.n, a.reps, rate)), flush=True)
        return 0
    import torch
    lines = [f"# tools/voxel_timing.py: {torch.cuda.get_device_name(0)}, HIP events, warm (back-to-back runs of one "
             f"cloud: what fits stays in the Infinity Cache), median of {a.reps}; stream rate {rate / 1e12:.2f} TB/s "
             f"(profiles/support_timing.txt); one child process per (cloud, size), {a.limit} s each"]
    print(lines[0], flush=True)
    for kind in CASES:
        for idx in range(len(CASES[kind][1])):
            cmd = [sys.executable, os.path.abspath(__file__), "--case", f"{kind}:{idx}", "--reps", str(a.reps), "--n", str(a.n)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"{kind}:{idx} ran over its {a.limit} s limit: stopping", flush=True)
                return 124
            if r.returncode != 0:
                print(f"{kind}:{idx} failed ({r.returncode}): stopping\n{r.stdout}{r.stderr}", flush=True)
                return r.returncode or 1
            lines += r.stdout.strip().splitlines()
            print(r.stdout.strip(), flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
