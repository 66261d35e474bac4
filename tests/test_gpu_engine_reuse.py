"""GPU: one engine's device buffers serve layouts of different sizes.

An engine's buffers only grow (csrc/pcm_host.hpp, DevBuf): a smaller cloud is
laid out in the buffers a larger one left behind, a larger one reallocates
them, ``reserve`` sizes the point buffers before the first layout, and
``close`` frees them all.  One engine fits 4,096, then 300, then 20,000
points; every fit must equal the CPU stand-in's (tests/cpu_engine.py, the
oracle behind the same driver) bit for bit.  D = 4 adds the coarse-list
buffers, PCM_ZLEV=2 the tile-box and tile-list buffers of a crowded layout.
K = 8, except in the crowded case: a tile gets a list of its own only in a
cell whose list is longer than TL_MIN = 16 (k_tile_cand), which 8 centres never
give, so that case takes tests/test_gpu_crowded.py's K = 256.  These clouds
have at most a few cells, each near all 256 centres: their lists overflow
CAPF = 64 (FULL) and every tile of theirs is listed, which the test asserts.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from cpu_engine import OracleEngine  # noqa: E402
from oracle import lloyd_ref as R  # noqa: E402
from test_gpu_parity import assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (4096, 300, 20000)
K, K_CROWDED, ITERS = 8, 256, 3
_refs = {}


@pytest.fixture(scope="module")
def pcm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pcm_amd
    return pcm_amd


def _case(pcm, n, d, k):
    """The cloud, its initial centres and the CPU engine's fit (computed once per shape, never modified)."""
    if (n, d, k) not in _refs:
        X = R.splitmix_uniform(n, d, seed=100 + d)
        C0 = X[R.init_indices(n, k)]
        res = pcm.lloyd_fit(torch.from_numpy(X), torch.from_numpy(C0), max_iter=ITERS, tol=0.0,
                            engine=OracleEngine(d, k, ITERS), group=pcm.lloyd.LOCAL)
        ref = dict(n_iter=res.n_iter, labels=res.labels.numpy(), centers=res.centers.numpy(),
                   changed=res.stat_words_changed, inertia=res.inertia)
        _refs[(n, d, k)] = (X, C0, ref)
    return _refs[(n, d, k)]


def _fit_all(pcm, eng, d, zlev, where):
    for n in SIZES:
        X, C0, ref = _case(pcm, n, d, eng.k)
        res = pcm.lloyd_fit(torch.from_numpy(X).cuda(), torch.from_numpy(C0).cuda(), max_iter=ITERS, tol=0.0,
                            engine=eng)
        torch.cuda.synchronize()
        st = eng.candidate_stats()
        print(where, n, d, eng.k, st)
        assert st.get("zlev", 0) == zlev, f"{where} n={n}"
        if zlev:   # the tile lists are written by k_tile_cand and read by k_lloyd1 / k_label
            assert st["crowded_tiles"] > 0 and st["listed_tiles"] > 0, f"{where} n={n}: {st}"
        assert_same(res, ref, f"{where} n={n} d={d}")


@pytest.mark.parametrize("d,zlev", [(3, 0), (4, 0), (3, 2)], ids=["d3", "d4-coarse-lists", "d3-crowded"])
def test_one_engine_across_layout_sizes(pcm, d, zlev, monkeypatch):
    from pcm_amd.engine import Engine
    if zlev:
        monkeypatch.setenv("PCM_ZLEV", str(zlev))   # read at every layout
    else:
        monkeypatch.delenv("PCM_ZLEV", raising=False)
    k = K_CROWDED if zlev else K
    eng = Engine(d, k, torch.float32, max_iter=ITERS)
    _fit_all(pcm, eng, d, zlev, "grown on demand")
    eng.close()
    eng = Engine(d, k, torch.float32, max_iter=ITERS)
    eng.reserve(max(SIZES))
    _fit_all(pcm, eng, d, zlev, "reserved")
    eng.close()
