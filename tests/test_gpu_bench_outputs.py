"""GPU: a plain ``bench.py`` run (no ``--full``) on a small cloud.

The result line carries the headline figures and none of ``--full``'s legs,
``--steps`` sets the number of timed iterations, and ``--dump-outputs`` holds
what the timed iterations ended with: the centres must be bitwise those of the
CPU oracle after warm-up + steps iterations of the same seeded cloud (the
engine and the oracle share the canonical arithmetic), the histories one entry
per iteration.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import lloyd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, D, WARMUP, STEPS = 200_000, 64, 3, 2, 3


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--n", str(N), "--k", str(K), "--d", str(D),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["full"] is False
    assert line["candidates"]["iterations"] == WARMUP + STEPS        # nothing iterated after the timed steps
    assert line["ms_per_step"] > 0 and line["unit"] == "point·iters/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32"
    assert abs(line["value"] - N / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    for leg in ("roofline", "breakdown_ms_per_iter", "fit", "kmeanspp_ms", "cpu_baseline", "cpu_numpy"):
        assert leg not in line, leg
    assert line["dumped_outputs"] == {"centers": [K, D], "center_shift": [WARMUP + STEPS],
                                      "stats_changed": [WARMUP + STEPS]}

    X = R.splitmix_uniform(N, D, seed=0)
    C0 = X[np.sort(np.random.default_rng(1).choice(N, K, replace=False))]
    ref = R.lloyd_fit(X, C0, max_iter=WARMUP + STEPS, tol=0.0, fast=True)
    assert ref["n_iter"] == WARMUP + STEPS
    centers = np.load(out / "centers.npy")
    assert centers.dtype == np.float32 and centers.shape == (K, D)
    assert np.array_equal(centers, ref["centers"])
    shift, changed = np.load(out / "center_shift.npy"), np.load(out / "stats_changed.npy")
    assert shift.dtype == changed.dtype == np.float64 and shift.shape == changed.shape == (WARMUP + STEPS,)
    assert np.all(shift > 0)
    np.testing.assert_array_equal(changed > 0, np.asarray(ref["changed"], dtype=np.int64) > 0)
