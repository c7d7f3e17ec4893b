"""The host model (comap_amd/csrc/cmx_host_{model,tree,verify}.cpp) built and run on its own, no GPU and no library:
tests/cpp/host_model_dump.cpp compiled with plain g++ -- that it compiles is the assertion that the three sources need no
HIP header -- and run over the case list of host_model_cases.py: every tree shape of the walk tests crossed with a model
for every layout the host builds.  Every valid case must pass the host's own self-check (verify_walk), the sizes of what
the device receives must follow from the dumped scalars, and an input that is wrong in two ways must be refused with the
message and the status code of the check that comes first.  scripts/compare_host_model.py compares the same dump, field by
field, between two versions of the sources."""
import os
import subprocess

import pytest

import host_model_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "comap_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "cpp", "host_model_dump")
SOURCES = ["cmx_host_model.cpp", "cmx_host_tree.cpp", "cmx_host_verify.cpp"]

# message and status code of every entry of host_model_cases.errors(), recorded from the sources before the host model was
# split (the first fault of each name is the one an earlier check finds)
EXPECTED_ERRORS = {
    "error/nstates_vs_postorder": (-2, "nstates must be between 2 and 64 (4 and 20 run on the matrix cores, the others on the plain kernels); got 65"),
    "error/nclasses_vs_ntypes": (-1, "nclasses out of range"),
    "error/Q_vs_incomplete_tree": (-1, "Q, pi, rates and probs are required"),
    "error/blen_vs_duplicate_taxon": (-1, "branch lengths must be finite and >= 0"),
    "error/unary_vs_probs": (-1, "internal nodes need at least two children"),
    "error/Qs_vs_rates": (-1, "non-homogeneous model: Qs, pis, model_of_branch and root_freqs are required"),
    "error/mob_vs_irreversible": (-1, "model_of_branch: generator index out of range"),
    "error/row_sum_in_generator_1": (-1, "rows of Q must sum to zero"),
}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """(valid names, error names, {case: {field: (length, value or None)} or ("error", code, message)})"""
    src = [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(ROOT, "tests", "cpp", "host_model_dump.cpp")]
    deps = src + [os.path.join(CSRC, h) for h in ("cmx_host_model.h", "cmx_host_parts.h", "cmx_layout.h", "cmx_walk.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + src + ["-o", EXE])
    cases = str(tmp_path_factory.mktemp("host_model") / "cases.txt")
    valid, bad = host_model_cases.write(cases)
    r = subprocess.run([EXE, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out, cur = {}, None
    for line in r.stdout.split("\n"):
        w = line.split()
        if line.startswith("case "):
            cur = w[1]
            out[cur] = {}
        elif line.startswith("error "):
            out[cur] = ("error", int(w[1]), line.split(" ", 2)[2])
        elif line:
            out[cur][w[0]] = (int(w[2]), int(w[4]) if len(w) > 4 else None)
    return valid, bad, out


def test_every_valid_case_builds_and_passes_the_self_check(dump):
    valid, _, out = dump
    assert len(valid) > 3000 and set(valid) <= set(out)
    refused = {n: out[n] for n in valid if isinstance(out[n], tuple)}
    assert not refused


def test_sizes_of_what_the_device_receives(dump):
    valid, _, out = dump
    checked = 0
    for name in valid:
        f = out[name]
        if f["plain"][1]:
            assert f["MAT"][0] == 0 and f["msched"][0] == 0 and f["nrec"][0] == 0, name
            continue
        dS = f["dS"][1]
        unit = (dS + (12 if dS == 4 else 4)) * (dS + 1)                     # mat_unit(dS), cmx_layout.h
        assert f["MAT"][0] == f["dC"][1] * f["MC"][1] * unit, name
        assert f["msched"][0] == 2 * (f["n_products"][1] + f["n_leaf_ops"][1]), name
        assert f["ldsched"][0] == f["n_loads"][1], name
        assert f["nrec"][0] == 16 * f["NV"][1], name
        checked += 1
    assert checked > 2500


def test_the_first_failing_check_decides_message_and_code(dump):
    _, bad, out = dump
    assert set(bad) == set(EXPECTED_ERRORS)
    for name, (code, message) in EXPECTED_ERRORS.items():
        assert out[name] == ("error", code, message), name
