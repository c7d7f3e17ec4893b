"""cmx::Mica::analyse (include/comap_mi355x_adapter.hpp) with nullMethod = "permutations" on a 61-state alignment writes the
bytes the Python mirror writes: both are thin over cmx_mi_columns, cmx_mica_average_mi and cmx_mica_permutation_test_states
(tests/cpp/adapter_mica_perm_main.cpp)."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import mica_perm_reference as ref
from comap_amd import engine, formats, mica

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adapter_mica_perm_main")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def perm_exe():
    src = os.path.join(ROOT, "tests", "cpp", "adapter_mica_perm_main.cpp")
    deps = [src, engine.LIB_PATH] + [os.path.join(ROOT, "include", h) for h in ("comap_mi355x_adapter.hpp", "comap_mi355x.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                               "-I", "/opt/rocm/include", src, "-o", EXE, "-L", os.path.dirname(engine.LIB_PATH),
                               "-lcomap_mi355x", "-L", "/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath," + os.path.dirname(engine.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_adapter_permutations_at_61_states_equal_the_python_mirror(perm_exe, tmp_path):
    A, T, N, max_perm, seed, first = 61, 40, 14, 130, 41, 10
    aln = ref.columns(A, T, N, 1000 * A + T)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<5i", T, N, A, max_perm, first) + struct.pack("<Q", seed) + np.ascontiguousarray(aln).tobytes())
    r = subprocess.run([perm_exe, str(inp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    res = mica.analysis(engine.Engine(), aln, nalpha=A, permutations=(max_perm, seed))
    buf = io.StringIO()
    formats.write_mica(buf, first + np.arange(N), res)
    assert r.stdout == buf.getvalue()
    assert r.stdout.split("\n")[0].endswith("Perm.p.value\tPerm.nb") and len(r.stdout.split("\n")) == N * (N - 1) // 2 + 2
