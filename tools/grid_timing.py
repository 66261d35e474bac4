"""Time ``pcm_height_grid`` (the exact height-map raster pass) against the PyTorch
route to the same planes on the same GPU in the same run: ``index_add_`` of
``[1, z]`` in float64 into a (G H W, 2) table plus ``scatter_reduce_`` ``amax`` and
``amin`` of z -- not exact (float adds in arrival order), and without the labels
the top and bottom words carry; the yardstick only.

Inputs: 14.4M points, fp32, K = 1024 labels (a 32 x 32 block pattern over the
image), G = 1 and G = 8 (the rows split into G contiguous clouds, as the plugin
concatenates the days), on

* the raster height-map cloud (the order the plugin delivers) at cell_log2 = 0
  (every lane its own pixel: the wave-uniform shortcut) and cell_log2 = 2 (runs
  of four lanes per cell: the segmented scan);
* the uniform cloud in generation order, scaled to the same image: neighbouring
  rows fall into unrelated pixels, one line per lane per atomic.

HIP events on the current stream, warm, median of ``reps`` back-to-back runs.
"kernel" is the buffer clear plus ``pcm_height_grid``; "torch" forms the pixel
keys and runs the three scatters into cleared tables, "scatters alone" has the
keys formed beforehand.  Each line gives the atomic floor -- 32 atomic bytes per
row at 1.3 TB/s, the rate measured for FLOAT atomics; nobody has measured 64-bit
integer atomics, so the floor is an ASSUMPTION -- and whether the words of two
different grid sizes are bit-equal.
usage: python tools/grid_timing.py [--out FILE] [--reps R]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcm_amd import _lib  # noqa: E402
from pcm_amd.engine import synth_uniform  # noqa: E402
from pcm_amd.fixed import fixed_q  # noqa: E402
from pcm_amd.grid import accumulate  # noqa: E402
from predict_timing import raster_cloud, timed  # noqa: E402

ATOMIC = 1.3e12   # B/s: float atomics (assumed to hold for 64-bit integer ones)
BYTES = 32.0      # atomic bytes per row: four 8-byte words


def case(name, X, side, s, reps, lines):
    n = X.shape[0]
    k = 1024
    H = W = (side - 1 >> s) + 1
    labels = ((X[:, 1] * (32.0 / side)).int().clamp_(0, 31) * 32 + (X[:, 2] * (32.0 / side)).int().clamp_(0, 31)).int()
    q = fixed_q([float(X[:, 0].abs().max())])[0]
    floor_ms = n * BYTES / ATOMIC * 1e3
    for G in (1, 8):
        g8 = None if G == 1 else (torch.arange(n, device="cuda") * G // n).to(torch.uint8)
        buf = torch.empty(G * 4 * H * W + 2, dtype=torch.int64, device="cuda")

        def kernel():
            buf.zero_()
            accumulate(X, labels, k, g8, G, (H, W), (0.0, 0.0), s, q, buf)
            return buf

        def keys():
            pix = torch.floor(torch.ldexp(X[:, 1], torch.tensor(-s, device="cuda"))).long() * W + \
                torch.floor(torch.ldexp(X[:, 2], torch.tensor(-s, device="cuda"))).long()
            return pix if G == 1 else g8.long() * (H * W) + pix

        def scatters(key):
            z = X[:, 0].double()
            table = torch.zeros(G * H * W, 2, dtype=torch.float64, device="cuda")
            table.index_add_(0, key, torch.stack([torch.ones_like(z), z], dim=1))
            hi = torch.full((G * H * W,), -float("inf"), dtype=torch.float64, device="cuda")
            lo = torch.full((G * H * W,), float("inf"), dtype=torch.float64, device="cuda")
            hi.scatter_reduce_(0, key, z, "amax")
            lo.scatter_reduce_(0, key, z, "amin")
            return table, hi, lo

        t_k, _ = timed(kernel, reps)
        words = buf.clone()
        t_r, (table, hi, lo) = timed(lambda: scatters(keys()), reps)
        key = keys()
        t_s, _ = timed(lambda: scatters(key), reps)
        # the words do not depend on the grid
        os.environ["PCM_GRID_BLOCKS"] = "97"
        kernel()
        equal = bool(torch.equal(buf, words))
        del os.environ["PCM_GRID_BLOCKS"]
        # and agree with the float tables: counts exactly, top and bottom to the truncation of one step of 2^-q
        w = words[:-2].view(G, 4, H * W)
        counts_ok = bool(torch.equal(w[:, 0].reshape(-1), table[:, 0].long()))
        seen = table[:, 0] > 0
        top = torch.ldexp(((w[:, 2] >> 32) - (1 << 25)).double(), torch.tensor(-q, device="cuda")).reshape(-1)
        bot = torch.ldexp(((1 << 25) - (w[:, 3] >> 32)).double(), torch.tensor(-q, device="cuda")).reshape(-1)
        dev = float(torch.maximum((top - hi)[seen].abs().max(), (bot - lo)[seen].abs().max()) * 2.0 ** q)
        lines.append(f"{name} n={n} cell_log2={s} raster {H}x{W} G={G}: kernel {t_k:.3f} ms ({floor_ms / t_k * 100:.1f} % of "
                     f"the {floor_ms:.3f} ms ASSUMED atomic floor: 32 B per row at the 1.3 TB/s of float atomics), torch "
                     f"float64 route {t_r:.3f} ms ({t_r / t_k:.1f}x), scatters alone {t_s:.3f} ms ({t_s / t_k:.1f}x), "
                     f"kernel beats the yardstick: {t_k < min(t_r, t_s)}; outside {int(words[-2])} skipped "
                     f"{int(words[-1])}; grids bit-equal: {equal}; counts equal torch's: {counts_ok}; top/bottom within "
                     f"{dev:.2f} steps of 2^-q")
        print(lines[-1], flush=True)
        del table, hi, lo, key, g8, buf, words, w, top, bot, seen
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    _lib.load()
    side = int(round(14_400_000 ** 0.5))
    lines = [f"# tools/grid_timing.py: {torch.cuda.get_device_name(0)}, HIP events, warm, median of {a.reps}; "
             f"K = 1024 labels in 32 x 32 blocks of the image"]
    X = raster_cloud(side)
    for s in (0, 2):
        case("raster height-map cloud", X, side, s, a.reps, lines)
    scale = torch.tensor([80.0, side, side], device="cuda")
    shift = torch.tensor([-40.0, 0.0, 0.0], device="cuda")
    X = (synth_uniform(side * side, 3, seed=0) * scale + shift).contiguous()
    X[:, 1:].clamp_(max=float(np.nextafter(np.float32(side), np.float32(0))))   # u * side may round up to side
    for s in (0, 2):
        case("uniform cloud (generation order)", X, side, s, a.reps, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
