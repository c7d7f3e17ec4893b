#!/usr/bin/env python3
"""The default mapping of a codon-sized alphabet on one GPU: cmx_map_sites_dev with every output, 61 states, Gamma 4,
synthetic.random_tree(64, 20260302), at (a) 2 000 sites -- the shape of README's plain-kernel row -- and (b) 64 000 sites, the
size of a null's launch.  Each shape runs the matrix-core path (cmx_map_wide.hip) and the forced plain path
(cmx_debug_map_wide_plain) alternated in one process; per path one warm-up call, then the median of --reps single calls
(device events around one call each) with the range.  Before the timing the two paths' results are compared.  Prints one
JSON line: both shapes, all four times, the two ratios and the two gates (a: plain / matrix-core >= 4; b: the matrix-core
median is not above the plain path's slowest call)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from comap_amd import engine, protein_models as pm, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sites", type=int, nargs="+", default=[2000, 64000])
ap.add_argument("--taxa", type=int, default=64)
ap.add_argument("--states", type=int, default=61)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--plain-reps", type=int, default=None, help="calls of the forced plain path per shape (default: --reps)")
a = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
dev = torch.device("cuda:0")
S = a.states
parent, blen, lot = synthetic.random_tree(a.taxa, 20260302)
Q, pi = pm.synthetic_reversible(S, 20260303)
rates, probs = pm.gamma_rates(0.5, 4)
eng = engine.Engine(parent, blen, lot, Q, pi, rates, probs)
was = engine.map_wide_plain(None)
out = {"workload": f"cmx_map_sites_dev, every output, {S} states, {a.taxa} taxa, Gamma 4", "shapes": []}
try:
    for n in a.sites:
        aln, _ = eng.simulate(20260304, 0, n)
        d_aln = torch.from_numpy(aln).to(dev)
        f64 = dict(dtype=torch.float64, device=dev)
        res = dict(counts=torch.zeros(eng.B * eng.K, n, **f64), logL=torch.zeros(n, **f64), post_rate=torch.zeros(n, **f64),
                   rate_class=torch.zeros(n, dtype=torch.int32, device=dev), norm=torch.zeros(n, **f64))

        def call(plain):
            engine.map_wide_plain(plain)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.map_sites_dev(d_aln, **res)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        call(True)                                       # (both calls are the warm-up of their path, too)
        ref = {k: v.clone() for k, v in res.items()}
        call(False)
        scale = float(ref["counts"].abs().max())
        diff = float((res["counts"] - ref["counts"]).abs().max()) / scale
        dlog = float((res["logL"] - ref["logL"]).abs().max())
        same_class = bool((res["rate_class"] == ref["rate_class"]).all())
        nplain = a.reps if a.plain_reps is None else a.plain_reps
        ms = {False: [], True: []}
        for r in range(max(a.reps, nplain)):
            for plain in (False, True):
                if r < (nplain if plain else a.reps):
                    ms[plain].append(call(plain))
        m, p = float(np.median(ms[False])), float(np.median(ms[True]))
        out["shapes"].append({"sites": n, "matrix_core_ms": m, "matrix_core_ms_min_max": [min(ms[False]), max(ms[False])],
                              "plain_ms": p, "plain_ms_min_max": [min(ms[True]), max(ms[True])], "plain_over_matrix_core": p / m,
                              "max_count_difference_over_largest_count": diff, "max_logL_difference": dlog,
                              "rate_classes_equal": same_class})
finally:
    engine.map_wide_plain(was)
sh = out["shapes"]
out["gate_a_at_least_4x"] = bool(sh[0]["plain_over_matrix_core"] >= 4.0)
if len(sh) > 1:
    out["gate_b_not_slower_than_plain_range"] = bool(sh[1]["matrix_core_ms"] <= sh[1]["plain_ms_min_max"][1])
print(json.dumps(out), flush=True)
