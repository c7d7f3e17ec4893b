#!/usr/bin/env python3
"""Mica's permutation test (null.method = permutations, CoMap/Mica.cpp:93-118) for codon-sized alphabets on one GPU: 2000
independent columns of 256 taxa (all 1 999 000 pairs), null.max_number_of_permutations = 1000, at 61 and 64 states -- fully
resolved, and with unknowns (code = A, 10 % of the symbols) in a tenth of the columns -- through
cmx_mica_permutation_test_states_dev.  In the same process: the 20-state call of scripts/bench_mica_perm.py (--shared 0),
the yardstick.  Every run is one warm-up call on 20 000 pairs and one timed call.  Prints one JSON line per run: pairs/s,
shuffles/s, mean shuffles per pair."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from comap_amd import engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2000)
ap.add_argument("--taxa", type=int, default=256)
ap.add_argument("--alphabets", type=int, nargs="+", default=[61, 64])
ap.add_argument("--max-perm", type=int, default=1000)
ap.add_argument("--shared", type=float, default=0.0, help="fraction of each column copied from a common ancestor column (0: independent columns)")
a = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
T, n = a.taxa, a.n
npairs = n * (n - 1) // 2
pv = torch.empty(npairs, dtype=torch.float64, device="cuda")
npm = torch.empty(npairs, dtype=torch.int32, device="cuda")
eng = engine.Engine()
lib, vp, sz = eng._lib, engine._vp, engine._sz


def bench(A, gap_columns, entry):
    rng = np.random.default_rng(20260103)
    base = rng.integers(0, A, size=(T, 1))
    aln = np.where(rng.random((T, n)) < a.shared, base, rng.integers(0, A, size=(T, n))).astype(np.uint8)
    if gap_columns > 0:
        cols = rng.random(n) < gap_columns
        aln[(rng.random((T, n)) < 0.10) & cols[None, :]] = A
    d = torch.from_numpy(aln).cuda()

    def run(p0, p1):
        eng._check(getattr(lib, entry)(eng._ctx, A, T, vp(d), sz(n), sz(n), ctypes.c_uint32(a.max_perm), ctypes.c_uint64(7), sz(p0),
                                       sz(p1), vp(pv), vp(npm), eng._stream()))

    run(0, min(npairs, 20000))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(0, npairs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    perms = int(npm.sum().item())
    print(json.dumps({"workload": f"mica permutation test: {n} columns ({npairs} pairs), {T} taxa, A={A}, max {a.max_perm}, "
                                  f"unknowns in {gap_columns:.0%} of the columns", "entry": entry, "seconds": dt,
                      "pairs_per_s": npairs / dt, "shuffles": perms, "shuffles_per_s": perms / dt,
                      "mean_shuffles_per_pair": perms / npairs, "median_pvalue": float(pv.median().item())}), flush=True)


bench(20, 0.0, "cmx_mica_permutation_test_dev")
for A in a.alphabets:
    bench(A, 0.0, "cmx_mica_permutation_test_states_dev")
    bench(A, 0.1, "cmx_mica_permutation_test_states_dev")
bench(20, 0.0, "cmx_mica_permutation_test_dev")
