#!/usr/bin/env python3
"""Price of per-branch weights (cmx_set_statistic_weights, DESIGN.md A.7, weighted) on one GPU, weighted and unweighted
runs alternated in one process after a warm-up of each, times from device events (median of --reps):
  * all pairs of 2 000 x 64-taxa protein sites, correlation (BASELINE configs[1]): cmx_pair_stats_dev;
  * the observed stage at the target (10 000 x 64): cmx_intra_compact_range_dev, compact records with a null's p-values;
  * the null at 125 replicates x 2 000 sites: weighted = unfused (simulate -> map -> score), unweighted = fused, with the
    device memory the weighted one adds (scratch growth at its first call);
  * how many entries of the unweighted outputs differ between before the first set and after a clear (expected 0).
Prints one JSON line."""
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
ap.add_argument("--null-reps", type=int, default=50, help="replicates x 10 000 sites of the null the p-values look up")
a = ap.parse_args()

dev = torch.device("cuda:0")
parent, blen, lot = synthetic.random_tree(64, 20260101)
mdl = synthetic.protein_model(0.5, 4)
eng = engine.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
B, K, N = eng.B, eng.K, 10000
rng = np.random.default_rng(20260105)
w = rng.uniform(0.0, 1.0, size=B) * blen[:B]          # e.g. weights by branch length, a few branches masked
w[rng.choice(B, size=B // 10, replace=False)] = 0.0
kind = engine.STAT_CORRELATION

aln = torch.empty((eng.T, N), dtype=torch.uint8, device=dev)
eng.simulate_dev(20260106, 0, N, aln)
counts = torch.empty((B * K, N), dtype=torch.float64, device=dev)
logL, pr, norm = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(3))
rc = torch.empty(N, dtype=torch.int32, device=dev)
eng.map_sites_dev(aln, counts, logL, pr, rc, norm)
c2k = counts[:, :2000].contiguous()
out2k = torch.empty((2000, 2000), dtype=torch.float64, device=dev)
nnull = a.null_reps * N
null_stat, null_nmin = (torch.empty(nnull, dtype=torch.float64, device=dev) for _ in range(2))
eng.null_intra_dev(kind, 20260107, 0, a.null_reps, N, null_stat, None, None, null_nmin)
npairs = N * (N - 1) // 2
comp = torch.empty(npairs * engine.PAIR_COMPACT.itemsize, dtype=torch.uint8, device=dev)
NR, RR = 125, 2000
ns = [torch.empty(NR * RR, dtype=torch.float64, device=dev) for _ in range(2)]
nm = torch.empty(NR * RR, dtype=torch.float64, device=dev)
pm = torch.empty(NR * RR, dtype=torch.float64, device=dev)
rcm = torch.empty(NR * RR, dtype=torch.int32, device=dev)
torch.cuda.synchronize()

stages = {
    "allpairs_2000x64": lambda: eng.pair_stats_dev(kind, c2k, out2k),
    "observed_compact_10000x64": lambda: eng.intra_compact_range_dev(kind, counts, norm, null_stat, null_nmin, 10, comp),
    "null_125x2000": lambda: eng.null_intra_dev(kind, 20260108, 0, NR, RR, ns[0], rcm, pm, nm),
}


def outputs():
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in (("allpairs", out2k), ("compact", comp), ("null", ns[0]))}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for f in stages.values():              # unweighted warm-up, then the reference outputs
    for _ in range(a.warmup):
        f()
before = outputs()
free0 = torch.cuda.mem_get_info(dev)[0]
eng.set_statistic_weights(w)
stages["null_125x2000"]()
torch.cuda.synchronize()
null_scratch = free0 - torch.cuda.mem_get_info(dev)[0]
for f in stages.values():
    for _ in range(a.warmup):
        f()
eng.set_statistic_weights(None)

res = {}
for name, f in stages.items():
    t = {"weighted": [], "unweighted": []}
    for r in range(a.reps):
        for mode in (("weighted", "unweighted") if r % 2 == 0 else ("unweighted", "weighted")):
            eng.set_statistic_weights(w if mode == "weighted" else None)
            t[mode].append(timed(f))
    eng.set_statistic_weights(None)
    mw, mu = float(np.median(t["weighted"])), float(np.median(t["unweighted"]))
    res[name] = {"weighted_ms": round(mw, 4), "unweighted_ms": round(mu, 4), "ratio": round(mw / mu, 4),
                 "weighted_ms_range": [round(min(t["weighted"]), 4), round(max(t["weighted"]), 4)],
                 "unweighted_ms_range": [round(min(t["unweighted"]), 4), round(max(t["unweighted"]), 4)]}
for f in stages.values():
    f()
after = outputs()
differ = {k: int(np.count_nonzero(before[k].view(np.uint8) != after[k].view(np.uint8))) for k in before}
res["null_125x2000"]["weighted_scratch_bytes"] = int(null_scratch)
print(json.dumps({"workload": "per-branch weights, 64-taxa protein JTT92+G4, correlation", "reps": a.reps, "stages": res,
                  "unweighted_bytes_differing_after_set_and_clear": differ, "nnull_for_pvalues": nnull,
                  "zero_weight_branches": int((w == 0).sum()), "nbranches": B}))
