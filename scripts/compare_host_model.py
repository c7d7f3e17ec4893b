#!/usr/bin/env python3
"""Compare what two versions of the host model build, field by field (the host analogue of compare_device_asm.py).

    scripts/compare_host_model.py OLD_CSRC NEW_CSRC [--keep DIR]

Builds tests/cpp/host_model_dump.cpp against the cmx_host_*.cpp of each directory with the same command
(hipcc -x hip --offload-host-only -O3 -std=c++17: it also builds a version whose host model still includes the device
header), writes the case list of tests/host_model_cases.py, runs both binaries and prints every case whose error line or
whose length / digest of a HostModel field differs.  Exit status 1 if any does.  It compares bytes only.
"""
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build(csrc, exe):
    src = sorted(glob.glob(os.path.join(csrc, "cmx_host_*.cpp"))) + [os.path.join(ROOT, "tests", "cpp", "host_model_dump.cpp")]
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-O3", "-std=c++17", "-I", csrc] + src + ["-o", exe])


def run(exe, cases):
    """{case: [lines]} in file order"""
    out, cur = {}, None
    for line in subprocess.check_output([exe, cases], text=True).split("\n"):
        if line.startswith("case "):
            cur = out.setdefault(line[5:], [])
        elif line:
            cur.append(line)
    return out


def main(argv):
    keep = None
    if "--keep" in argv:
        keep = argv[argv.index("--keep") + 1]
        argv = [a for a in argv if a not in ("--keep", keep)]
    if len(argv) != 2:
        sys.exit(__doc__)
    import host_model_cases
    work = keep or tempfile.mkdtemp(prefix="cmx_host_model_")
    os.makedirs(work, exist_ok=True)
    try:
        cases = os.path.join(work, "cases.txt")
        valid, bad = host_model_cases.write(cases)
        sides = []
        for tag, csrc in zip(("old", "new"), argv):
            exe = os.path.join(work, "host_model_dump_" + tag)
            build(os.path.abspath(csrc), exe)
            sides.append(run(exe, cases))
        old, new = sides
        differing, fields = 0, 0
        for name in valid + bad:
            a, b = old.get(name), new.get(name)
            if a is None or b is None:
                print("MISSING  %s" % name)
                differing += 1
                continue
            fields += max(len(a), len(b)) if not a[0].startswith("error") else 0
            if a != b:
                differing += 1
                keys = sorted(set(l.split()[0] for l in set(a) ^ set(b)))
                print("DIFFERS  %s: %s" % (name, ", ".join(keys) if not (a[0] + b[0]).count("error") else "%r / %r" % (a[0], b[0])))
        failed = [n for n in valid if old.get(n, ["error"])[0].startswith("error")]
        for n in failed:
            print("REFUSED by the old sources  %s: %s" % (n, old[n][0]))
        print("%d cases (%d valid, %d errors), %d fields compared: %d cases differ" % (len(valid) + len(bad), len(valid), len(bad), fields, differing))
        return 1 if differing or failed else 0
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
