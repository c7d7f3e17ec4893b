"""CMX_SCRATCH_GUARD over the window index (cmx_window_null_dev and the calls that read it), as tests/test_gpu_scratch_guard.py does
for the other stages: every scratch buffer of the build and of the queries carries a canary behind its last byte, at a ragged size."""
import numpy as np
import pytest
import torch

from comap_amd import engine
from comap_amd.pipeline import IntraAnalysis
from conftest import make_case
from window_reference import window_test

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def guard():
    was = engine.scratch_guard(True)          # before any context of this module is created
    engine.scratch_guard_failures(clear=True)
    yield
    engine.scratch_guard(was)


def _clean(eng):
    eng.synchronize()
    eng.scratch_check()
    assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()


def test_window_index_build_and_queries_under_the_guard():
    eng = engine.Engine()
    rng = np.random.default_rng(41)
    ns, nm = rng.normal(size=4099), rng.gamma(2.0, 1.0, size=4099)
    ns[rng.integers(0, 4099, 30)] = np.nan
    s, m = rng.normal(size=257), rng.uniform(0, 6, size=257)
    got = eng.window_test(ns, nm, s, m, window=0.2, min_nobs=3)
    ref = window_test(ns, nm, s, m, 0.2, min_nobs=3)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0], equal_nan=True)
    _clean(eng)
    eng.window_test(ns[:33], nm[:33], s, m, window=1.0)        # a smaller null in the first one's buffers: the canaries move
    eng.window_test([], [], s, m)
    _clean(eng)


def test_window_pair_loop_under_the_guard():
    case = make_case(8, 37, 20, 91)
    eng = engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    ana = IntraAnalysis(eng, torch.from_numpy(case["aln"]).cuda(), engine.STAT_CORRELATION)
    ana.get_vectors()
    nb = ana.null_distribution(5, 0, 3, 37)
    ana.compute_intra_window(nb["stat"], nb["nmin"], 0.2)
    ana.prefetch_intra_gram(3, 30)
    ana.compute_intra_window(nb["stat"], nb["nmin"], 0.2, True, 3, 30)
    _clean(eng)
