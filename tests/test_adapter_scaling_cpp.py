"""cmx::Engine::setLikelihoodScaling / getLikelihoodScaling (include/comap_mi355x_adapter.hpp): the C++ mirror of
cmx_set_likelihood_scaling.  On a tree beyond fp64's range the adapter's marginal ancestral states, scaled, are the Python
engine's byte for byte and finite -- both are thin over the same C-ABI calls (tests/cpp/adapter_scaling_main.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import scaled_cases as sc
from comap_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adapter_scaling_main")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scaling_exe():
    src = os.path.join(ROOT, "tests", "cpp", "adapter_scaling_main.cpp")
    deps = [src, engine.LIB_PATH] + [os.path.join(ROOT, "include", h) for h in ("comap_mi355x_adapter.hpp", "comap_mi355x.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                               "-I", "/opt/rocm/include", src, "-o", EXE, "-L", os.path.dirname(engine.LIB_PATH),
                               "-lcomap_mi355x", "-L", "/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath," + os.path.dirname(engine.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_adapter_scaled_ancestral_states_equal_the_python_engine(scaling_exe, tmp_path):
    from test_adapter_cpp import _write_case
    c = sc.long(20, 300)
    case = dict(parent=c.parent, blen=c.blen, lot=c.lot, Q=c.Q, pi=c.pi, rates=c.rates, probs=c.probs, aln=c.aln)
    N, S = c.aln.shape[1], 20
    inp, out = tmp_path / "in.bin", tmp_path / "o.bin"
    _write_case(inp, case, N, 1, 1, 1, 1)
    r = subprocess.run([scaling_exe, str(inp), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    before, after, ni = np.frombuffer(raw, dtype="<i4", count=3)
    assert (before, after) == (0, 1)
    states = np.frombuffer(raw, dtype=np.uint8, count=ni * N, offset=12).reshape(ni, N)
    probs = np.frombuffer(raw, dtype="<f8", count=ni * N * S, offset=12 + ni * N).reshape(ni, N, S)
    eng = c.engine()
    eng.set_likelihood_scaling(True)
    ref = eng.ancestral_states(c.aln, want_posterior=True)
    assert ni == len(ref["nodes"]) and np.isfinite(probs).all()
    assert np.array_equal(states, ref["states"]) and np.array_equal(probs, ref["post"])
