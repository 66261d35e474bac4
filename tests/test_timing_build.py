"""CPU: the timing build of the Lloyd engine's host units compiles and links.

The per-block phase stamps (``-DPCM_DBG_TIMING``, csrc/pcm_debug.hpp, read by
tools/*_timing.py) are compiled by no product build, so a kernel edit can break
them unnoticed: a stamp in front of loads that are pinned to scalar registers
once did ("illegal VGPR to SGPR copy" in k_updlists).  This compiles every unit
that came out of csrc/pcm_engine.hip ("host units"), host and device,
with the product flags plus that define, and links them into one shared object:
the stamp arrays are per unit, so a second definition of one of them, or of a
kernel of a shared header, shows here as a duplicate symbol.
"""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from pcm_amd import _lib

ENGINE_UNITS = ("pcm_engine.hip", "pcm_layout.hip", "pcm_kpp.hip", "pcm_predict.hip", "pcm_inspect.hip", "pcm_cloud.hip")
# the read-backs of the stamp arrays, each defined by the unit whose kernels write the copy it reads
READERS = ("pcm_debug_timing", "pcm_debug_timing_lloyd", "pcm_debug_timing_kpp", "pcm_debug_timing_eval",
           "pcm_debug_kpp_counts")


@pytest.mark.slow
def test_engine_units_compile_and_link_with_phase_stamps(tmp_path):
    if not os.path.exists(_lib.HIPCC):
        pytest.skip("hipcc not available")
    units = [u for u in _lib.UNITS if os.path.basename(u) in ENGINE_UNITS]
    assert len(units) == len(ENGINE_UNITS), units
    inc = ["-I", os.path.join(_lib.REPO_DIR, "include")]
    objs = [str(tmp_path / (os.path.basename(u) + ".o")) for u in units]
    cmds = [[_lib.HIPCC, *_lib.HIP_FLAGS[:-1], *inc, "-DPCM_DBG_TIMING", "-c", u, "-o", o] for u, o in zip(units, objs)]
    with ThreadPoolExecutor(max_workers=min(len(cmds), os.cpu_count() or 1)) as ex:
        for cmd, r in zip(cmds, ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), cmds)):
            assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr[-4000:]}"
    so = str(tmp_path / "libpcm_timing.so")
    link = [_lib.HIPCC, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", so, *objs]
    r = subprocess.run(link, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(link)}\n{r.stderr[-4000:]}"
    nm = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not [s for s in READERS if s not in defined]
