"""cmx::MarginalAncestralStateReconstruction (include/comap_mi355x_adapter.hpp), the stand-in for CoMap.cpp:169-197: its
states (getAncestralSequences) and posteriors (getAncestralStatesForNode(node, probs)) equal the Python engine's byte for
byte -- both are thin over cmx_ancestral_states (tests/cpp/adapter_ancestral_main.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from comap_amd import engine
from conftest import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adapter_ancestral_main")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ancestral_exe():
    src = os.path.join(ROOT, "tests", "cpp", "adapter_ancestral_main.cpp")
    deps = [src, engine.LIB_PATH] + [os.path.join(ROOT, "include", h) for h in ("comap_mi355x_adapter.hpp", "comap_mi355x.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                               "-I", "/opt/rocm/include", src, "-o", EXE, "-L", os.path.dirname(engine.LIB_PATH),
                               "-lcomap_mi355x", "-L", "/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath," + os.path.dirname(engine.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


@pytest.mark.parametrize("S,seed", [(20, 19), (4, 23)])
def test_adapter_states_and_probs_equal_the_python_engine(ancestral_exe, tmp_path, S, seed):
    from test_adapter_cpp import _write_case
    case = make_case(13, 150, S, seed)
    N = 150
    inp, out = tmp_path / "in.bin", tmp_path / "o.bin"
    _write_case(inp, case, N, 1, 1, 1, 1)
    r = subprocess.run([ancestral_exe, str(inp), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    ni = int(np.frombuffer(raw, dtype="<i4", count=1)[0])
    nodes = np.frombuffer(raw, dtype="<i4", count=ni, offset=4)
    off = 4 + 4 * ni
    states = np.frombuffer(raw, dtype=np.uint8, count=ni * N, offset=off).reshape(ni, N)
    off += ni * N
    probs = np.frombuffer(raw, dtype="<f8", count=ni * N * S, offset=off).reshape(ni, N, S)
    off += 8 * ni * N * S
    assert np.frombuffer(raw, dtype="<i4", count=1, offset=off)[0] == 1, "a leaf must be rejected"
    eng = engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    ref = eng.ancestral_states(case["aln"], want_posterior=True)
    assert list(nodes) == ref["nodes"]
    assert np.array_equal(states, ref["states"])
    assert np.array_equal(probs, ref["post"])
