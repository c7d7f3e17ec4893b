"""Per-branch weights through the C++ mirror of the reference interface (include/comap_mi355x_adapter.hpp) and the
multi-GPU driver (include/comap_mi355x_multigpu.hpp): Statistic::setWeights / Distance::setWeights give what the Python
engine gives with the same weights, a weights vector of the wrong size throws DimensionException, and a LoopbackMultiGpu
run with weights equals the single-context path byte for byte (tests/cpp/adapter_weights_main.cpp)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from comap_amd import engine
from conftest import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adapter_weights_main")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def weights_exe():
    src = os.path.join(ROOT, "tests", "cpp", "adapter_weights_main.cpp")
    deps = [src, engine.LIB_PATH] + [os.path.join(ROOT, "include", h) for h in
                                      ("comap_mi355x_multigpu.hpp", "comap_mi355x_adapter.hpp", "comap_mi355x.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                               "-I", "/opt/rocm/include", src, "-o", EXE, "-L", os.path.dirname(engine.LIB_PATH),
                               "-lcomap_mi355x", "-L", "/opt/rocm/lib", "-lrccl", "-lamdhip64",
                               "-Wl,-rpath," + os.path.dirname(engine.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def _write(path, case, N, rep_cpu, rep_ram, ncls, seed, w):
    from test_adapter_cpp import _write_case
    _write_case(path, case, N, rep_cpu, rep_ram, ncls, seed)
    with open(path, "ab") as f:
        f.write(struct.pack("<i", len(w)) + np.asarray(w, dtype=np.float64).tobytes())


def _weights(B, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.1, 2.0, size=B)
    w[[1, B // 2]] = 0.0
    return w


def test_statistic_and_distance_weights_equal_the_python_engine(weights_exe, tmp_path):
    case = make_case(10, 60, 20, 17)
    N = 60
    eng = engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    B = eng.B
    w = _weights(B, 5)
    inp, out = tmp_path / "in.bin", tmp_path / "o.bin"
    _write(inp, case, N, 1, 1, 1, 1, w)
    subprocess.check_call([weights_exe, "dists", str(inp), str(out)])
    raw = np.fromfile(out, dtype="<f8", count=N * B + B + 4 * N * N)
    counts = raw[:N * B].reshape(N, B, 1)
    wn = raw[N * B:N * B + B]
    cor, dcomp, deuc, cor_unw = raw[N * B + B:].reshape(4, N, N)
    dim = np.frombuffer(open(out, "rb").read()[-8:], dtype="<i4")
    assert list(dim) == [1, 1], "a weights vector of the wrong size must throw DimensionException"
    m = eng.map_sites(case["aln"])
    assert np.array_equal(counts, m["counts"])
    assert np.allclose(wn, w / w.sum(), rtol=1e-15, atol=0)      # getWeights: the copy divided by its sum
    eng.set_statistic_weights(wn)      # what the adapter hands the context: the statistic's normalised copy
    iu = np.triu_indices(N, 1)
    pc = eng.pair_stats(engine.STAT_CORRELATION, counts)
    pm = eng.pair_stats(engine.STAT_COMPENSATION, counts)
    pe = eng.pair_stats(engine.STAT_EUCLIDIAN_DISTANCE, counts)
    eng.set_statistic_weights(None)
    assert np.array_equal(cor[iu], pc[iu])
    assert np.array_equal(dcomp[iu], 1.0 - pm[iu])
    assert np.array_equal(deuc[iu], pe[iu])
    assert np.array_equal(cor_unw[iu], eng.pair_stats(engine.STAT_CORRELATION, counts)[iu])
    assert not np.array_equal(cor[iu], cor_unw[iu])


@pytest.mark.parametrize("nranks,rep_cpu,rep_ram,nsites", [(2, 5, 37, 70)])
def test_loopback_two_ranks_with_weights_equal_the_single_context(weights_exe, tmp_path, nranks, rep_cpu, rep_ram, nsites):
    case = make_case(9, nsites, 20, 63)
    ncls, seed = 5, 4300
    eng = engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    w = _weights(eng.B, 8)
    inp, out = tmp_path / "in.bin", tmp_path / "o.bin"
    _write(inp, case, nsites, rep_cpu, rep_ram, ncls, seed, w)
    r = subprocess.run([weights_exe, "loopback", str(inp), str(out), str(nranks)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    nrows = struct.unpack_from("<q", raw, 0)[0]
    rec = np.dtype([("i", "<i8"), ("j", "<i8"), ("stat", "<f8"), ("pr", "<f8"), ("nm", "<f8"), ("pv", "<f8"),
                    ("rc", "<i4"), ("ns", "<i4")])
    assert nrows == nsites * (nsites - 1) // 2
    rows = np.frombuffer(raw, dtype=rec, count=nrows, offset=8)
    off = 8 + nrows * rec.itemsize
    nnull = struct.unpack_from("<q", raw, off)[0]
    nstat = np.frombuffer(raw, dtype="<f8", count=nnull, offset=off + 8)
    nnmin = np.frombuffer(raw, dtype="<f8", count=nnull, offset=off + 8 + 8 * nnull)
    eng.set_statistic_weights(w)
    nl = eng.null_intra(engine.STAT_CORRELATION, seed, 0, rep_cpu, rep_ram)
    assert np.array_equal(nstat, nl["stat"], equal_nan=True) and np.array_equal(nnmin, nl["nmin"], equal_nan=True)
    m = eng.map_sites(case["aln"])
    ref, count = eng.intra_rows(engine.STAT_CORRELATION, m["counts"], m["rate_class"], m["post_rate"], m["norm"], nl["stat"],
                                nl["nmin"], nclasses=ncls)
    eng.set_statistic_weights(None)
    assert count == nrows
    for a, b in (("i", "i"), ("j", "j"), ("stat", "stat"), ("pr", "pr_min"), ("nm", "n_min"), ("pv", "pvalue"), ("rc", "rc_min"), ("ns", "nsim")):
        assert np.array_equal(rows[a], ref[b], equal_nan=True), a
    unw = eng.null_intra(engine.STAT_CORRELATION, seed, 0, rep_cpu, rep_ram)
    assert not np.array_equal(unw["stat"], nstat)
