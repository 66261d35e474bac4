"""Time ``local_moments`` / ``point_normals`` step by step -- ``pcm_nearest_keys``, the ``torch.sort``
calls, the gather of the cell-sorted targets, the scan kernel ``k_moments`` (``PCM_MOMENTS_PHASE``
runs the last two apart) and ``k_moments_planes`` -- on the same GPU in the same run as its
yardsticks:

* ``k_support`` on the target cloud and ``k_nearest`` on the same pair of clouds at the same radius:
  the same scan with cheaper inner loops (a count; a 64-bit minimum) and 4 or 8 bytes of output per
  row instead of 80; the ratios are reported, and k_support's mean neighbour count is printed with
  every case as the measure of the candidates a query meets;
* a floor: the bytes of the sorted copy (24 B per target row: three float and three int32 planes)
  read 27/8 times -- the 27 cells around a row, a staged candidate taken to serve 8 rows, as
  tools/nearest_timing.py takes it -- plus 80 B per query row written, at the stream rate measured
  here (``sum`` of a 2 GiB float32 buffer, far larger than the 256 MB Infinity Cache);
* a chunked PyTorch float64 brute force (256 queries against all targets per step: the float32
  predicate written out, the raw float64 moments by one matrix product, moved to the query) at a
  size it can finish: the first 65 536 queries against 1M targets of a 1M x 1M pair, where the kernels
  are timed on all of it and counts (exactly), mean offsets and covariances (to float64 rounding) are
  compared.

Inputs: 14.4M points, fp32, tools/nearest_timing.py's clouds: the raster height-map cloud queried by
a second day of it, and the uniform cloud queried by a second draw; two radii each, for about 5 and
about 30 neighbours per row; and the raster cloud against itself (``targets=None``: one key pass,
one sort).

Every case runs in its own child process under its own time limit -- a fresh interpreter, not a
replaced one --, and the run stops at the first child that fails.  HIP events on the current
stream, warm, median of ``reps`` back-to-back runs: the sorted copy of 14.4M targets is 346 MB, of
which what one repeat left in the 256 MB Infinity Cache serves the next, so every figure here ran
WARM in it.
usage: python tools/moments_timing.py [--out FILE] [--reps R] [--n N]
"""
import argparse
import os
import subprocess
import sys

ROW_BYTES = 24.0
OUT_BYTES = 80.0
READS = 27.0 / 8.0
BRUTE_QUERIES = 65_536                  # the float64 brute force is quadratic: this many queries against all targets
CASES = (                               # name, the child's time limit in seconds
    ("rate", 120),
    ("yardstick:raster:1.8", 300),
    ("steps:raster:1.8", 240), ("steps:raster:3.6", 240),
    ("steps:uniform:4.57", 240), ("steps:uniform:8.3", 240),
    ("self:raster:1.8", 240),
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
    from pcm_amd import _lib, moments, nearest, support
    from pcm_amd.engine import synth_uniform
    from nearest_timing import SHIFT
    from predict_timing import raster_cloud, timed

    _lib.load()
    kind, *rest = a.case.split(":")

    if kind == "rate":
        buf = torch.ones(1 << 29, dtype=torch.float32, device="cuda")      # 2 GiB
        t, _ = timed(lambda: buf.sum(), a.reps)
        rate = buf.numel() * 4 / (t * 1e-3)
        print(f"# tools/moments_timing.py: {torch.cuda.get_device_name(0)}, HIP events, warm (back-to-back runs of one "
              f"pair of clouds: what a repeat leaves of the sorted copy in the Infinity Cache serves the next), median of "
              f"{a.reps}; stream rate {rate / 1e12:.2f} TB/s (sum of 2 GiB); MOMENTS_CHUNK {_lib.MOMENTS_CHUNK}; every case "
              f"in its own process")
        print(f"RATE {rate!r}")
        return

    def clouds(which, side):
        """-> (queries, targets): tools/nearest_timing.py's later and earlier cloud."""
        if which == "raster":
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

    def phase(name, value):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(value)

    def steps(X, Y, r):
        """``Y`` None: one cloud.  -> (ms of keys, sorts, gather, k_moments, k_moments_planes, local_moments, point_normals;
        the PointNormals; ms of k_support and of k_nearest; k_support's mean count)."""
        r32 = np.float32(r)
        T = X if Y is None else Y
        n, m = X.shape[0], T.shape[0]
        t_keys, (xkeys, ykeys, info) = timed(lambda: nearest.nearest_keys(X, X[:0] if Y is None else Y, r32), a.reps)
        t_sort, (sx, sy) = timed(lambda: (torch.sort(xkeys), (None, None) if Y is None else torch.sort(ykeys)), a.reps)
        q = moments.default_q(moments._maxabs(X, Y), m, r32)
        ws = moments.workspace(m, X.device)
        words = torch.zeros((n, _lib.MOMENTS_WORDS), dtype=torch.int64, device="cuda")
        call = lambda: moments.moments_scan(X, Y, r32, q, sx[0], sx[1], sy[0], sy[1], info, ws, words)  # noqa: E731
        phase("PCM_MOMENTS_PHASE", 1)
        t_gather, _ = timed(call, a.reps)
        phase("PCM_MOMENTS_PHASE", 2)
        t_scan, _ = timed(call, a.reps)
        phase("PCM_MOMENTS_PHASE", None)
        t_planes, _ = timed(lambda: moments.moments_planes(words, q, 3), a.reps)
        t_lm, lm = timed(lambda: moments.local_moments(X, r, targets=Y), a.reps)
        assert torch.equal(lm.words, words) and lm.q == q
        del lm
        t_pn, pn = timed(lambda: moments.point_normals(X, r, targets=Y), a.reps)
        # k_nearest on the same pair of clouds and radius (the targets' sort is made here when there is one cloud)
        sy = sx if Y is None else sy
        nws = nearest.workspace(m, X.device)
        index = torch.empty(n, dtype=torch.int32, device="cuda")
        sq = torch.empty(n, dtype=torch.float32, device="cuda")
        if Y is None:
            xkeys, ykeys, ninfo = nearest.nearest_keys(X, X, r32)
        else:
            ninfo = info
        find = lambda: nearest.nearest_find(X, T, None, None, r32, sx[0], sx[1], sy[0], sy[1], ninfo, nws, index, sq)  # noqa: E731
        phase("PCM_NEAREST_PHASE", 1)
        find()
        phase("PCM_NEAREST_PHASE", 2)
        t_near, _ = timed(find, a.reps)
        phase("PCM_NEAREST_PHASE", None)
        del xkeys, ykeys, sx, sy, ws, nws
        # k_support on the targets at the same radius
        keys, sinfo = support.support_keys(T, r32)
        skeys, perm = torch.sort(keys)
        counts = torch.empty(m, dtype=torch.int32, device="cuda")
        sws = support.workspace(m, T.device)
        phase("PCM_SUPPORT_PHASE", 1)
        support.support_count(T, None, 1, r32, -1, skeys, perm, sinfo, sws, counts, None)
        phase("PCM_SUPPORT_PHASE", 2)
        t_sup, _ = timed(lambda: support.support_count(T, None, 1, r32, -1, skeys, perm, sinfo, sws, counts, None), a.reps)
        phase("PCM_SUPPORT_PHASE", None)
        return (t_keys, t_sort, t_gather, t_scan, t_planes, t_lm, t_pn), pn, t_sup, t_near, float(counts.double().mean())

    def brute_force(X, Y, r, rows=256):
        """Chunked PyTorch float64 brute force -> (count int64 (n,), mean offset (n, 3), covariance (n, 6)) of the
        float32 predicate's neighbourhoods, zz, zy, zx, yy, yx, xx."""
        r2 = torch.tensor(np.float32(r) * np.float32(r), device="cuda")
        n = X.shape[0]
        z, y, x = (Y[:, c].contiguous() for c in range(3))
        Yd = Y.double()
        pa, pb = (0, 0, 0, 1, 1, 2), (0, 1, 2, 1, 2, 2)
        F = torch.cat([torch.ones_like(Yd[:, :1]), Yd, Yd[:, pa] * Yd[:, pb]], dim=1)          # (m, 10)
        count = torch.empty(n, dtype=torch.int64, device="cuda")
        mean = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        cov = torch.empty((n, 6), dtype=torch.float64, device="cuda")
        for s in range(0, n, rows):
            e = min(n, s + rows)
            dz, dy, dx = X[s:e, 0:1] - z[None, :], X[s:e, 1:2] - y[None, :], X[s:e, 2:3] - x[None, :]
            near = ((dz * dz + dy * dy) + dx * dx) <= r2
            raw = near.double() @ F                                        # the raw moments about the origin
            c = raw[:, 0:1]
            mu = raw[:, 1:4] / c
            count[s:e] = raw[:, 0].round().long()
            mean[s:e] = mu - X[s:e].double()
            cov[s:e] = raw[:, 4:10] / c - mu[:, pa] * mu[:, pb]
        return count, mean, cov

    which, r = rest[0], float(rest[1])
    if kind == "yardstick":
        side = int(round(min(a.n, 1_000_000) ** 0.5))
        X, Y = clouds(which, side)
        (t_keys, t_sort, t_gather, t_scan, t_planes, t_lm, t_pn), pn, t_sup, t_near, mean_count = steps(X, Y, r)
        brute_force(X[:1024], Y, r)                                      # warm: allocator, code objects
        part = min(X.shape[0], BRUTE_QUERIES)
        t_bf, (count, mean, cov) = timed(lambda: brute_force(X[:part], Y, r), 1)
        lm = pn.moments
        has = count > 0
        d_mu = float((lm.offsets()[:part] - mean)[has].abs().max())
        C = lm.covariances()[:part]
        mine = torch.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], dim=1)
        d_cov = float((mine - cov)[has].abs().max())
        print(f"yardstick, {which} cloud {X.shape[0]} x {Y.shape[0]} r={r} (k_support counts {mean_count:.1f} neighbours per "
              f"target, q {lm.q}, cell_log2 {lm.cell_log2}): chunked PyTorch float64 brute force of the first {part} "
              f"queries {t_bf:.1f} ms (one run after its warm-up; {t_bf * X.shape[0] / part:.0f} ms at that rate for all), "
              f"local_moments of all queries as a whole {t_lm:.3f} ms ({t_bf * X.shape[0] / part / t_lm:.0f}x; keys {t_keys:.3f}, sorts "
              f"{t_sort:.3f}, gather {t_gather:.3f}, k_moments {t_scan:.3f} ms), point_normals as a whole {t_pn:.3f} ms "
              f"(k_moments_planes {t_planes:.3f} ms); counts equal: {bool(torch.equal(count, lm.counts()[:part]))}, largest "
              f"difference of a mean offset {d_mu:.3e}, of a covariance entry {d_cov:.3e} (the brute force sums float64 "
              f"about the origin, coordinates up to {float(Y.abs().max()):.0f}; the words quantise at 2^-q)")
        return

    side = int(round(a.n ** 0.5))
    X, Y = clouds(which, side)
    if kind == "self":
        X, Y = Y, None
    (t_keys, t_sort, t_gather, t_scan, t_planes, t_lm, t_pn), pn, t_sup, t_near, mean_count = steps(X, Y, r)
    n, m = X.shape[0], (X if Y is None else Y).shape[0]
    floor_ms = (m * ROW_BYTES * READS + n * OUT_BYTES) / a.rate * 1e3
    valid = float(pn.valid().double().mean()) * 100
    print(f"{which} cloud {n} x {m}{' (one cloud, targets=None)' if Y is None else ''} r={r} (k_support counts "
          f"{mean_count:.1f} neighbours per target, mean count {float(pn.count.double().mean()):.1f}, {valid:.1f} % of the rows "
          f"have a plane, q {pn.moments.q}, cell_log2 {pn.moments.cell_log2}): keys {t_keys:.3f} ms, sort"
          f"{'' if Y is None else 's'} {t_sort:.3f} ms, gather {t_gather:.3f} ms, k_moments {t_scan:.3f} ms "
          f"({floor_ms / t_scan * 100:.1f} % of the {floor_ms:.3f} ms floor: 24 B per target read 27/8 times and 80 B per "
          f"query written at the measured {a.rate / 1e12:.2f} TB/s; {t_scan / t_sup:.2f}x k_support's {t_sup:.3f} ms on the "
          f"targets, {t_scan / t_near:.2f}x k_nearest's {t_near:.3f} ms on the same pair), k_moments_planes {t_planes:.3f} "
          f"ms, local_moments as a whole {t_lm:.3f} ms, point_normals as a whole {t_pn:.3f} ms")


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
