"""CPU: the timing build of the engine unit compiles.

The per-block phase stamps (``-DPCM_DBG_TIMING``, csrc/pcm_debug.hpp, read by
tools/*_timing.py) are compiled by no product build, so a kernel edit can break
them unnoticed: a stamp in front of loads that are pinned to scalar registers
once did ("illegal VGPR to SGPR copy" in k_updlists).  This compiles
csrc/pcm_engine.hip device-only with the product flags plus that define.
"""
import os
import subprocess

import pytest

from pcm_amd import _lib


@pytest.mark.slow
def test_engine_unit_compiles_with_phase_stamps(tmp_path):
    if not os.path.exists(_lib.HIPCC):
        pytest.skip("hipcc not available")
    unit = next(u for u in _lib.UNITS if u.endswith("pcm_engine.hip"))
    cmd = [_lib.HIPCC, *_lib.HIP_FLAGS[:-1], "-I", os.path.join(_lib.REPO_DIR, "include"), "-DPCM_DBG_TIMING",
           "--cuda-device-only", "-c", unit, "-o", str(tmp_path / "pcm_engine_timing.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr[-4000:]}"
