#!/usr/bin/env python3
"""Price of per-site likelihood scaling (cmx_set_likelihood_scaling) on one GPU: cmx_map_sites_dev with
every output, three ways in one process on the same device -- scaled on the matrix-core kernels of cmx_map_wide.hip /
cmx_map_wide20.hip (the default), scaled on the plain kernels (cmx_debug_map_scaled_plain: the yardstick, device text
unchanged) and unscaled -- times from device events after a warm-up (median of --reps), at three shapes:
  * 2 000 sites x 64 taxa, protein JTT92 + Gamma4: unscaled is the matrix-core walk;
  * 2 000 sites x 64 taxa, 61 states + Gamma4: unscaled is the wide mapping;
  * 2 000 sites x 600 and x 1 000 taxa, protein (unscaled is timed too, but underflows there);
and cmx_null_intra_dev of --null-reps replicates x 1 000 pairs at 600 taxa, scaled, both ways.
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from comap_amd import engine, protein_models as pm, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--null-reps", type=int, default=3)
a = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def median(fn):
    for _ in range(a.warmup):
        fn()
    t = [timed(fn) for _ in range(a.reps)]
    return round(float(np.median(t)), 4), [round(min(t), 4), round(max(t), 4)]


def shape(name, ntaxa, nsites, nstates, seed, null=False):
    parent, blen, lot = synthetic.random_tree(ntaxa, seed)
    mdl = synthetic.protein_model(0.5, 4)
    if nstates != 20:
        mdl["Q"], mdl["pi"] = pm.synthetic_reversible(nstates, seed)
    try:        # (the walk's workspaces are allocated with the context, scaling or not: DESIGN.md 4.5.5)
        eng = engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    except engine.CmxError as e:
        return name, {"sites": nsites, "taxa": ntaxa, "error": str(e)}
    N = nsites
    aln = torch.empty((eng.T, N), dtype=torch.uint8, device=dev)
    eng.simulate_dev(seed + 1, 0, N, aln)
    counts = torch.empty((eng.B * eng.K, N), dtype=torch.float64, device=dev)
    logL, pr, norm = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(3))
    rc = torch.empty(N, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    out = {"sites": N, "taxa": ntaxa, "states": eng.S, "classes": eng.C}
    for key, on, plain in (("unscaled", False, False), ("scaled_plain", True, True), ("scaled", True, False)):
        eng.set_likelihood_scaling(on)
        engine.map_scaled_plain(plain)
        t, r = median(lambda: eng.map_sites_dev(aln, counts, logL, pr, rc, norm))
        torch.cuda.synchronize()
        out[key + "_ms"], out[key + "_ms_range"] = t, r
        out[key + "_finite_sites"] = int(torch.isfinite(logL).sum().item())
    out["scaled_over_unscaled"] = round(out["scaled_ms"] / out["unscaled_ms"], 2)
    out["scaled_plain_over_scaled"] = round(out["scaled_plain_ms"] / out["scaled_ms"], 2)
    if null:   # the unfused null that scaling selects: simulate, map, score, per replicate
        ram = 1000
        stat, prmin, nmin = (torch.empty(a.null_reps * ram, dtype=torch.float64, device=dev) for _ in range(3))
        rcmin = torch.empty(a.null_reps * ram, dtype=torch.int32, device=dev)
        for key, plain in (("null_scaled_plain", True), ("null_scaled", False)):
            engine.map_scaled_plain(plain)
            fn = lambda: eng.null_intra_dev(engine.STAT_CORRELATION, 9, 0, a.null_reps, ram, stat, rcmin, prmin, nmin)  # noqa: E731
            fn()
            t = [timed(fn) for _ in range(3)]
            out[key + "_ms"], out[key + "_ms_range"] = round(float(np.median(t)), 3), [round(min(t), 3), round(max(t), 3)]
            out[key + "_nan"] = int(torch.isnan(stat).sum().item())
        out["null_replicates"], out["null_pairs_per_replicate"] = a.null_reps, ram
        out["null_scaled_plain_over_scaled"] = round(out["null_scaled_plain_ms"] / out["null_scaled_ms"], 2)
    return name, out


was = engine.map_scaled_plain(None)
try:
    res = dict(shape(*s) for s in (("2000x64_protein", 64, 2000, 20, 20260301),
                                     ("2000x64_61states", 64, 2000, 61, 20260302),
                                     ("2000x600_protein", 600, 2000, 20, 20260303, True),
                                     ("2000x1000_protein", 1000, 2000, 20, 20260304)))
finally:
    engine.map_scaled_plain(was)
print(json.dumps({"workload": "cmx_map_sites_dev, every output, Gamma4: scaled on the matrix-core kernels, scaled on the plain "
                  "kernels, unscaled; cmx_null_intra_dev at 600 taxa scaled both ways", "reps": a.reps, "shapes": res}))
