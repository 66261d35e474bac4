"""Time ``radius_support`` step by step -- ``pcm_support_keys``, ``torch.sort`` of the keys, the
gather of the cell-sorted copy and the count kernel ``k_support`` (``PCM_SUPPORT_PHASE`` runs
the last two apart) -- on the same GPU in the same run as its two yardsticks:

* the chunked PyTorch brute force (512 rows against all rows per step, the float32 predicate
  written out) at a size it can finish: 1M points of the same kind of cloud, where the kernel
  is timed too and the counts are compared;
* a floor: the bytes of the sorted copy (13 B per row) read 27/8 times -- the 27 cells around a
  row, a staged candidate taken to serve 8 rows -- at the stream rate measured here (``sum`` of a 2 GiB float32 buffer, far larger than the 256 MB
  Infinity Cache).

Inputs: 14.4M points, fp32: the raster height-map cloud in the order the plugin delivers, and
the uniform cloud in generation order scaled to the same box; two radii each, chosen for about
5 and about 30 neighbours per row (the measured mean is printed); G = 1 and G = 4 (the rows
split into G contiguous clouds).  HIP events on the current stream, warm, median of ``reps``
back-to-back runs: the sorted copy of 14.4M rows is 187 MB and stays in the Infinity Cache
between repeats, so every figure here ran WARM in it.
usage: python tools/support_timing.py [--out FILE] [--reps R] [--n N]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcm_amd import _lib, support  # noqa: E402
from pcm_amd.engine import synth_uniform  # noqa: E402
from predict_timing import raster_cloud, timed  # noqa: E402

ROW_BYTES = 13.0
READS = 27.0 / 8.0


def emit(lines, out, text):
    lines.append(text)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def stream_rate(reps):
    buf = torch.ones(1 << 29, dtype=torch.float32, device="cuda")      # 2 GiB
    t, _ = timed(lambda: buf.sum(), reps)
    return buf.numel() * 4 / (t * 1e-3)


def phase(value):
    if value is None:
        os.environ.pop("PCM_SUPPORT_PHASE", None)
    else:
        os.environ["PCM_SUPPORT_PHASE"] = str(value)


def steps(X, r, G, reps):
    """-> (ms of keys, sort, gather, count, the whole call; counts; days or None; cell_log2)."""
    n = X.shape[0]
    r32 = np.float32(r)
    g8 = None if G == 1 else (torch.arange(n, device="cuda") * G // n).to(torch.uint8)
    t_keys, (keys, info) = timed(lambda: support.support_keys(X, r32), reps)
    t_sort, (skeys, perm) = timed(lambda: torch.sort(keys), reps)
    ws = support.workspace(n, X.device)
    counts = torch.empty(n, dtype=torch.int32, device="cuda")
    days = torch.empty(n, dtype=torch.int32, device="cuda") if g8 is not None else None
    call = lambda: support.support_count(X, g8, G, r32, -1, skeys, perm, info, ws, counts, days)   # noqa: E731
    phase(1)
    t_gather, _ = timed(call, reps)
    phase(2)
    t_count, _ = timed(call, reps)
    phase(None)
    t_all, sup = timed(lambda: support.radius_support(X, r, groups=g8, n_groups=G if g8 is not None else None), reps)
    assert torch.equal(sup.counts, counts) and (days is None or torch.equal(sup.days, days))
    return (t_keys, t_sort, t_gather, t_count, t_all), counts, days, int(info[0])


def brute_force(X, r, rows=512):
    """Chunked PyTorch brute force of the same predicate -> int32 counts."""
    r2 = torch.tensor(np.float32(r) * np.float32(r), device="cuda")
    n = X.shape[0]
    z, y, x = (X[:, a].contiguous() for a in range(3))
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    for a in range(0, n, rows):
        b = min(n, a + rows)
        dz, dy, dx = z[a:b, None] - z[None, :], y[a:b, None] - y[None, :], x[a:b, None] - x[None, :]
        out[a:b] = ((dz * dz + dy * dy) + dx * dx <= r2).sum(1, dtype=torch.int32) - 1
    return out


def case(name, X, radii, rate, reps, lines, out):
    n = X.shape[0]
    floor_ms = n * ROW_BYTES * READS / rate * 1e3
    for r in radii:
        for G in (1, 4):
            (t_keys, t_sort, t_gather, t_count, t_all), counts, days, s = steps(X, r, G, reps)
            mean = float(counts.double().mean())
            emit(lines, out,
                 f"{name} n={n} r={r} (mean {mean:.1f} neighbours, max {int(counts.max())}, cell_log2 {s}) G={G}: keys "
                 f"{t_keys:.3f} ms, sort {t_sort:.3f} ms, gather {t_gather:.3f} ms, count {t_count:.3f} ms "
                 f"({floor_ms / t_count * 100:.1f} % of the {floor_ms:.3f} ms floor: 13 B per row read 27/8 times at the "
                 f"measured {rate / 1e12:.2f} TB/s), radius_support as a whole {t_all:.3f} ms"
                 + ("" if days is None else f"; rows seen by all {G} groups: {int((days == G).sum())}"))
            del counts, days
    torch.cuda.empty_cache()


def yardstick(name, X, r, reps, lines, out):
    n = X.shape[0]
    (t_keys, t_sort, t_gather, t_count, t_all), counts, _, s = steps(X, r, 1, reps)
    brute_force(X[:4096], r)                                         # warm: allocator, code objects
    t_bf, ref = timed(lambda: brute_force(X, r), 1)
    emit(lines, out,
         f"yardstick, {name} n={n} r={r} (mean {float(counts.double().mean()):.1f} neighbours, cell_log2 {s}): chunked "
         f"PyTorch brute force {t_bf:.1f} ms (one run after its warm-up), radius_support as a whole {t_all:.3f} ms "
         f"({t_bf / t_all:.0f}x; keys {t_keys:.3f}, sort {t_sort:.3f}, gather {t_gather:.3f}, count {t_count:.3f} ms); "
         f"counts equal: {bool(torch.equal(ref, counts))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=14_400_000)
    a = ap.parse_args()
    _lib.load()
    lines = []
    rate = stream_rate(a.reps)
    emit(lines, a.out,
         f"# tools/support_timing.py: {torch.cuda.get_device_name(0)}, HIP events, warm (back-to-back runs of one "
         f"cloud: its 187 MB sorted copy stays in the Infinity Cache), median of {a.reps}; stream rate "
         f"{rate / 1e12:.2f} TB/s (sum of 2 GiB); SUPPORT_CHUNK {_lib.SUPPORT_CHUNK}")
    side = int(round(a.n ** 0.5))
    small = int(round(min(a.n, 1_000_000) ** 0.5))
    scale = torch.tensor([80.0, 1.0, 1.0], device="cuda")
    shift = torch.tensor([-40.0, 0.0, 0.0], device="cuda")

    def uniform(sd):
        return (synth_uniform(sd * sd, 3, seed=0) * (scale * torch.tensor([1.0, sd, sd], device="cuda")) + shift).contiguous()

    # the yardsticks first, at 1M points: the radii of "about 5 neighbours"
    yardstick("raster height-map cloud", raster_cloud(small), 1.8, a.reps, lines, a.out)
    yardstick("uniform cloud (generation order)", uniform(small), 4.57, a.reps, lines, a.out)
    case("raster height-map cloud", raster_cloud(side), (1.8, 3.6), rate, a.reps, lines, a.out)
    case("uniform cloud (generation order)", uniform(side), (4.57, 8.3), rate, a.reps, lines, a.out)


if __name__ == "__main__":
    main()
