#!/usr/bin/env python3
"""Mica column MI for codon-sized alphabets on one GPU: two alignments of 2000 + 2000 columns, 256 taxa, all 4e6 cross pairs,
at 61 and 64 states, in three cases -- no unknowns, unknowns (code = A, 5 % of the rows) in a tenth of the columns, and in
every column.  Every case runs the matrix-core path and the forced plain path (cmx_debug_mica_wide_plain) alternated in
one process; per path the median of --reps single calls (device events around one call each).  Before the timing the two
paths' results are compared.  Prints one JSON line per (A, case)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from comap_amd import engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n1", type=int, default=2000)
ap.add_argument("--n2", type=int, default=2000)
ap.add_argument("--taxa", type=int, default=256)
ap.add_argument("--alphabets", type=int, nargs="+", default=[61, 64])
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
dev = torch.device("cuda:0")
T = a.taxa
eng = engine.Engine()
mi = torch.empty((a.n1, a.n2), dtype=torch.float64, device=dev)
hj = torch.empty_like(mi)
h1 = torch.empty(a.n1, dtype=torch.float64, device=dev)
h2 = torch.empty(a.n2, dtype=torch.float64, device=dev)
was = engine.mica_wide_plain(None)
try:
    for A in a.alphabets:
        for case, frac in (("no unknowns", 0.0), ("unknowns in a tenth of the columns", 0.1), ("unknowns in every column", 1.0)):
            rng = np.random.default_rng(20260103)
            base = rng.integers(0, A, size=(T, 1))
            a1 = np.where(rng.random((T, a.n1)) < 0.6, base, rng.integers(0, A, size=(T, a.n1))).astype(np.uint8)
            a2 = np.where(rng.random((T, a.n2)) < 0.4, base, rng.integers(0, A, size=(T, a.n2))).astype(np.uint8)
            for arr in (a1, a2):
                cols = rng.random(arr.shape[1]) < frac
                arr[(rng.random(arr.shape) < 0.05) & cols[None, :]] = A
            d1, d2 = torch.from_numpy(a1).to(dev), torch.from_numpy(a2).to(dev)

            def call(plain):
                engine.mica_wide_plain(plain)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.mi_columns_dev(d1, mi, hj, d2, A, None, h1, h2)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)

            call(True)
            ref = mi.clone(), hj.clone()
            call(False)                                  # (both calls are the warm-up of their path, too)
            diff = max(float((mi - ref[0]).abs().max()), float((hj - ref[1]).abs().max()))
            ident = float((mi - (h1[:, None] + h2[None, :] - hj)).abs().max())
            ms = {False: [], True: []}
            for _ in range(a.reps):
                for plain in (False, True):
                    ms[plain].append(call(plain))
            pairs = a.n1 * a.n2
            m, p = float(np.median(ms[False])), float(np.median(ms[True]))
            print(json.dumps({"workload": f"mica {a.n1}x{a.n2} columns, {T} taxa, A={A}, {case}", "pairs": pairs,
                              "matrix_core_ms": m, "matrix_core_pairs_per_s": pairs / m * 1e3,
                              "matrix_core_ms_min_max": [min(ms[False]), max(ms[False])],
                              "plain_ms": p, "plain_pairs_per_s": pairs / p * 1e3, "plain_ms_min_max": [min(ms[True]), max(ms[True])],
                              "plain_over_matrix_core": p / m, "max_abs_difference_of_the_paths": diff,
                              "max_identity_residual": ident}), flush=True)
finally:
    engine.mica_wide_plain(was)
