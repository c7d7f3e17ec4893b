#!/usr/bin/env python3
"""Price of the marginal ancestral states (asr.method = marginal, cmx_ancestral_states_dev) on one GPU,
times from device events after a warm-up (median of --reps), at three shapes:
  * target: 10 000 sites x 64 taxa, protein JTT92 + Gamma4;
  * cfg4:   10 000 sites x 256 taxa, DNA GTR + Gamma4;
  * cfg2:    2 000 sites x 64 taxa, protein JTT92 + Gamma4.
Next to each: the observed mapping (cmx_map_sites_dev, every output) at the same shape, the passes, and the algorithmic
scratch traffic -- the four per-node vectors written once (4 C nn S N doubles) plus the two read back per internal node
(2 C n_inner S N) -- over the time.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from comap_amd import engine, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
dev = torch.device("cuda:0")
BUDGET = 2 << 30      # kAsrScratchBytes (cmx_api_map.cpp)


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


def shape(name, ntaxa, nsites, protein, seed):
    parent, blen, lot = synthetic.random_tree(ntaxa, seed)
    mdl = synthetic.protein_model(0.5, 4) if protein else synthetic.dna_model(0.5, 4)
    eng = engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    S, C, nn, N = eng.S, eng.C, len(parent), nsites
    nin = len(eng.inner_nodes())
    aln = torch.empty((eng.T, N), dtype=torch.uint8, device=dev)
    eng.simulate_dev(seed + 1, 0, N, aln)
    states = torch.empty((nin, N), dtype=torch.uint8, device=dev)
    post = torch.empty((nin, S, N), dtype=torch.float64, device=dev)
    counts = torch.empty((eng.B * eng.K, N), dtype=torch.float64, device=dev)
    logL, pr, norm = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(3))
    rc = torch.empty(N, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t_states, r_states = median(lambda: eng.ancestral_states_dev(aln, states))
    t_post, r_post = median(lambda: eng.ancestral_states_dev(aln, states, post))
    t_map, r_map = median(lambda: eng.map_sites_dev(aln, counts, logL, pr, rc, norm))
    per_site = 8 * 4 * C * nn * S
    max_chunk = max(256, BUDGET // per_site // 256 * 256)
    passes = -(-N // max_chunk)
    traffic = 8 * C * S * N * (4 * nn + 2 * nin)
    return name, {"sites": N, "taxa": ntaxa, "states": S, "classes": C, "inner_nodes": nin, "passes": passes,
                  "sites_per_pass": min(N, (-(-N // passes) + 255) // 256 * 256),
                  "asr_states_ms": t_states, "asr_states_ms_range": r_states,
                  "asr_with_posterior_ms": t_post, "asr_with_posterior_ms_range": r_post,
                  "map_sites_dev_ms": t_map, "map_sites_dev_ms_range": r_map,
                  "scratch_traffic_bytes": traffic, "scratch_traffic_GBps": round(traffic / (t_states * 1e-3) / 1e9, 1)}


res = dict(shape(*s) for s in (("target_10000x64_protein", 64, 10000, True, 20260201),
                                 ("cfg4_10000x256_dna", 256, 10000, False, 20260202),
                                 ("cfg2_2000x64_protein", 64, 2000, True, 20260203)))
print(json.dumps({"workload": "marginal ancestral states (asr.method = marginal), Gamma4", "reps": a.reps, "shapes": res}))
