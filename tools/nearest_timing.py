"""Time ``nearest_points`` step by step -- ``pcm_nearest_keys``, the two ``torch.sort`` calls, the
gather of the cell-sorted targets and the scan kernel ``k_nearest`` (``PCM_NEAREST_PHASE`` runs
the last two apart) -- on the same GPU in the same run as its yardsticks:

* the chunked PyTorch brute force (256 queries against all targets per step, the float32
  predicate written out, the lowest row among the minima) at a size it can finish: 1M x 1M points
  of the same kind of cloud, where the kernel is timed too and index and distance are compared
  for equality;
* ``k_support`` on the target cloud at the same radius: the same scan with a cheaper inner loop
  (a count instead of a 64-bit minimum); the ratio is reported, and its mean neighbour count is
  printed with every case as the measure of the candidates a query meets;
* a floor: the bytes of the sorted copy (16 B per target row: three planes and the row number)
  read 27/8 times -- the 27 cells around a row, a staged candidate taken to serve 8 rows, as
  tools/support_timing.py takes it -- at the stream rate measured here (``sum`` of a 2 GiB
  float32 buffer, far larger than the 256 MB Infinity Cache).

Inputs: 14.4M points, fp32.  The raster height-map cloud in the order the plugin delivers, queried
by a second day of it -- its own noise, shifted by a sub-pixel motion --, and the uniform cloud in
generation order scaled to the same box, queried by a second draw; two radii each, chosen for
about 5 and about 30 candidates per query.  The last case is a whole ``kmeans_assign(change=)``
from host arrays (wall clock: the copies to the device, the labelling and the lookup).

Every case runs in its own child process under its own time limit -- a fresh interpreter, not a
replaced one --, and the run stops at the first child that fails.  HIP events on the current
stream, warm, median of ``reps`` back-to-back runs: the sorted copy of 14.4M targets is 230 MB and
stays in the Infinity Cache between repeats, so every figure here ran WARM in it.
usage: python tools/nearest_timing.py [--out FILE] [--reps R] [--n N]
"""
import argparse
import os
import subprocess
import sys
import time

ROW_BYTES = 16.0
READS = 27.0 / 8.0
SHIFT = (0.11, 0.37, -0.29)            # the second day's motion against the first: z, y, x in pixels
CASES = (                               # name, the child's time limit in seconds
    ("rate", 120),
    ("yardstick:raster:1.8", 420), ("yardstick:uniform:4.57", 420),
    ("steps:raster:1.8", 240), ("steps:raster:3.6", 240),
    ("steps:uniform:4.57", 240), ("steps:uniform:8.3", 240),
    ("assign:raster:1.8", 420),
)


def parent(a):
    lines, rate = [], None
    here = os.path.abspath(__file__)

    def emit(text):
        lines.append(text)
        print(text, flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for name, limit in CASES:
        cmd = [sys.executable, here, "--case", name, "--reps", str(a.reps), "--n", str(a.n)]
        if rate is not None:
            cmd += ["--rate", repr(rate)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            emit(f"# {name}: ended at its {limit} s limit; nothing further was run")
            return 1
        out = [ln for ln in r.stdout.splitlines() if ln.strip()]
        if r.returncode != 0:
            emit(f"# {name}: exit status {r.returncode}; nothing further was run\n# " +
                 "\n# ".join((r.stderr or "").strip().splitlines()[-5:]))
            return 1
        for ln in out:
            if ln.startswith("RATE "):
                rate = float(ln.split()[1])
            else:
                emit(ln)
    return 0


# ---------------------------------------------------------------- the children
def child(a):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from pcm_amd import _lib, nearest, support
    from pcm_amd.engine import synth_uniform
    from predict_timing import raster_cloud, timed

    _lib.load()
    kind, *rest = a.case.split(":")

    if kind == "rate":
        buf = torch.ones(1 << 29, dtype=torch.float32, device="cuda")      # 2 GiB
        t, _ = timed(lambda: buf.sum(), a.reps)
        rate = buf.numel() * 4 / (t * 1e-3)
        print(f"# tools/nearest_timing.py: {torch.cuda.get_device_name(0)}, HIP events, warm (back-to-back runs of one "
              f"pair of clouds: the 230 MB sorted copy of the targets stays in the Infinity Cache), median of {a.reps}; "
              f"stream rate {rate / 1e12:.2f} TB/s (sum of 2 GiB); NEAREST_CHUNK {_lib.NEAREST_CHUNK}; every case in "
              f"its own process")
        print(f"RATE {rate!r}")
        return

    def clouds(which, side):
        """-> (queries, targets): the later and the earlier cloud."""
        if which == "raster":
            # the earlier day is predict_timing's raster cloud; the later day samples the same relief at
            # the moved pixel centres, with its own noise
            yy, xx = torch.meshgrid(torch.arange(side, device="cuda", dtype=torch.float32) + SHIFT[1],
                                    torch.arange(side, device="cuda", dtype=torch.float32) + SHIFT[2], indexing="ij")
            g = torch.Generator(device="cuda").manual_seed(1)
            z = 40 * torch.sin(xx / 230.0) + 25 * torch.cos(yy / 170.0) + SHIFT[0] + \
                torch.randn(xx.shape, device="cuda", generator=g)
            return torch.stack([z, yy, xx], dim=-1).reshape(-1, 3).contiguous(), raster_cloud(side)
        scale = torch.tensor([80.0, float(side), float(side)], device="cuda")
        shift = torch.tensor([-40.0, 0.0, 0.0], device="cuda")
        return ((synth_uniform(side * side, 3, seed=1) * scale + shift).contiguous(),
                (synth_uniform(side * side, 3, seed=0) * scale + shift).contiguous())

    def phase(value):
        if value is None:
            os.environ.pop("PCM_NEAREST_PHASE", None)
        else:
            os.environ["PCM_NEAREST_PHASE"] = str(value)

    def steps(X, Y, r):
        """-> (ms of keys, the two sorts, gather, k_nearest, the whole call; the Nearest; k_support's ms and mean)."""
        r32 = np.float32(r)
        n, m = X.shape[0], Y.shape[0]
        t_keys, (xkeys, ykeys, info) = timed(lambda: nearest.nearest_keys(X, Y, r32), a.reps)
        t_sort, (sx, sy) = timed(lambda: (torch.sort(xkeys), torch.sort(ykeys)), a.reps)
        ws = nearest.workspace(m, X.device)
        index = torch.empty(n, dtype=torch.int32, device="cuda")
        sq = torch.empty(n, dtype=torch.float32, device="cuda")
        call = lambda: nearest.nearest_find(X, Y, None, None, r32, sx[0], sx[1], sy[0], sy[1], info, ws, index, sq)  # noqa: E731
        phase(1)
        t_gather, _ = timed(call, a.reps)
        phase(2)
        t_scan, _ = timed(call, a.reps)
        phase(None)
        t_all, near = timed(lambda: nearest.nearest_points(X, Y, r), a.reps)
        assert torch.equal(near.index, index) and torch.equal(near.sqdist, sq)
        del xkeys, ykeys, sx, sy, ws
        # k_support on the targets at the same radius: the same scan with a cheaper inner loop
        keys, sinfo = support.support_keys(Y, r32)
        skeys, perm = torch.sort(keys)
        counts = torch.empty(m, dtype=torch.int32, device="cuda")
        sws = support.workspace(m, Y.device)
        os.environ["PCM_SUPPORT_PHASE"] = "1"
        support.support_count(Y, None, 1, r32, -1, skeys, perm, sinfo, sws, counts, None)
        os.environ["PCM_SUPPORT_PHASE"] = "2"
        t_sup, _ = timed(lambda: support.support_count(Y, None, 1, r32, -1, skeys, perm, sinfo, sws, counts, None), a.reps)
        os.environ.pop("PCM_SUPPORT_PHASE")
        return (t_keys, t_sort, t_gather, t_scan, t_all), near, t_sup, float(counts.double().mean())

    def brute_force(X, Y, r, rows=256):
        """Chunked PyTorch brute force of the same predicate and tie rule -> (int32 index, float32 sqdist)."""
        r2 = torch.tensor(np.float32(r) * np.float32(r), device="cuda")
        inf = torch.tensor(float("inf"), device="cuda")
        n, m = X.shape[0], Y.shape[0]
        z, y, x = (Y[:, c].contiguous() for c in range(3))
        cols = torch.arange(m, dtype=torch.int32, device="cuda")
        none = torch.tensor(2 ** 31 - 1, dtype=torch.int32, device="cuda")
        index = torch.empty(n, dtype=torch.int32, device="cuda")
        sq = torch.empty(n, dtype=torch.float32, device="cuda")
        for s in range(0, n, rows):
            e = min(n, s + rows)
            dz, dy, dx = X[s:e, 0:1] - z[None, :], X[s:e, 1:2] - y[None, :], X[s:e, 2:3] - x[None, :]
            d2 = (dz * dz + dy * dy) + dx * dx
            d2 = torch.where(d2 <= r2, d2, inf)
            best = d2.amin(1)
            first = torch.where(d2 == best[:, None], cols[None, :], none).amin(1)      # the lowest row among the minima
            found = best <= r2
            index[s:e] = torch.where(found, first, torch.full_like(first, -1))
            sq[s:e] = best
        return index, sq

    if kind == "yardstick":
        which, r = rest[0], float(rest[1])
        side = int(round(min(a.n, 1_000_000) ** 0.5))
        X, Y = clouds(which, side)
        (t_keys, t_sort, t_gather, t_scan, t_all), near, t_sup, mean = steps(X, Y, r)
        brute_force(X[:1024], Y, r)                                      # warm: allocator, code objects
        t_bf, (index, sq) = timed(lambda: brute_force(X, Y, r), 1)
        print(f"yardstick, {which} cloud {X.shape[0]} x {Y.shape[0]} r={r} (k_support counts {mean:.1f} neighbours per target, "
              f"{float(near.found().double().mean()) * 100:.1f} % found, cell_log2 {near.cell_log2}): chunked PyTorch "
              f"brute force {t_bf:.1f} ms (one run after its warm-up), nearest_points as a whole {t_all:.3f} ms "
              f"({t_bf / t_all:.0f}x; keys {t_keys:.3f}, sorts {t_sort:.3f}, gather {t_gather:.3f}, k_nearest "
              f"{t_scan:.3f} ms); index equal: {bool(torch.equal(index, near.index))}, distance equal: "
              f"{bool(torch.equal(sq, near.sqdist))}")
        return

    side = int(round(a.n ** 0.5))
    which, r = rest[0], float(rest[1])
    X, Y = clouds(which, side)
    if kind == "steps":
        (t_keys, t_sort, t_gather, t_scan, t_all), near, t_sup, mean = steps(X, Y, r)
        floor_ms = Y.shape[0] * ROW_BYTES * READS / a.rate * 1e3
        print(f"{which} cloud {X.shape[0]} x {Y.shape[0]} r={r} (k_support counts {mean:.1f} neighbours per target, "
              f"{float(near.found().double().mean()) * 100:.1f} % found, cell_log2 {near.cell_log2}): keys {t_keys:.3f} ms, "
              f"two sorts {t_sort:.3f} ms, gather {t_gather:.3f} ms, k_nearest {t_scan:.3f} ms ({floor_ms / t_scan * 100:.1f} % "
              f"of the {floor_ms:.3f} ms floor: 16 B per target read 27/8 times at the measured {a.rate / 1e12:.2f} TB/s; "
              f"{t_scan / t_sup:.2f}x k_support's {t_sup:.3f} ms on the targets at this radius), nearest_points as a "
              f"whole {t_all:.3f} ms")
        return
    if kind == "assign":
        from pcm_amd import plugin
        early, late = Y.cpu().numpy().astype(np.float64), X.cpu().numpy().astype(np.float64)
        del X, Y
        torch.cuda.empty_cache()
        pick = np.sort(np.random.default_rng(1).choice(early.shape[0], 1024, replace=False))
        model = dict(centers=early[pick])
        plugin.kmeans_assign([late[:100_000]], model, change=r, change_to=early[:100_000])     # warm
        t0 = time.perf_counter()
        _, res = plugin.kmeans_assign([late], model)
        t1 = time.perf_counter()
        _, res = plugin.kmeans_assign([late], model, change=r, change_to=early)
        t2 = time.perf_counter()
        print(f"kmeans_assign of the {late.shape[0]}-point {which} day from host float64 arrays, K = 1024 (wall clock, "
              f"one run after a warm-up): {(t1 - t0) * 1e3:.0f} ms without change=, {(t2 - t1) * 1e3:.0f} ms with "
              f"change={r} against the {early.shape[0]}-point earlier day ({res['change']['found'].mean() * 100:.1f} % "
              f"found, median change {np.nanmedian(res['change']['distance']):.3f})")
        return
    raise SystemExit(f"unknown case {a.case!r}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=14_400_000)
    ap.add_argument("--case", default=None, help="internal: run one case in this process")
    ap.add_argument("--rate", type=float, default=0.0, help="internal: the measured stream rate in B/s")
    a = ap.parse_args()
    sys.exit(parent(a) if a.case is None else child(a))


if __name__ == "__main__":
    main()
