#!/usr/bin/env python3
"""The fused null with and without its pattern path (cmx_set_null_patterns) on a bench.py workload: launch time of
cmx_null_intra_dev on simulated alignments supplied as bench.py supplies them, the number of distinct columns mapped, and
the worst case -- supplied alignments whose columns are all distinct.  Both paths must give the same bytes.
usage (GPU box, repo root): python scripts/time_null_patterns.py [target|cfg3|cfg4] [reps]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from comap_amd import engine as E

wl = sys.argv[1] if len(sys.argv) > 1 else "target"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
w = bench.WORKLOADS[wl]
parent, blen, lot, mdl, Bk, clamp = bench.build_inputs(w)
eng = E.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk=Bk, clamp_negative=clamp)
kind = E.STAT_BY_NAME[w["statistic"]]
nrep, ram, T = w["nrep"](1), w["rep_ram"], eng.T
n = nrep * ram
dev = torch.device("cuda:0")
sim = torch.empty(nrep * 2 * T * ram, dtype=torch.uint8, device=dev)
eng.null_simulate_dev(w["seed"] + 7, 0, nrep, ram, sim)
g = torch.Generator(device=dev)
g.manual_seed(5)
distinct = torch.randint(0, eng.S, (nrep * 2 * T * ram,), dtype=torch.uint8, device=dev, generator=g)
out = {k: torch.empty(n, dtype=torch.int32 if k == "rcmin" else torch.float64, device=dev) for k in ("stat", "rcmin", "prmin", "nmin")}
res = dict(workload=wl, sites=2 * n)
for name, sup in (("simulated", sim), ("all_distinct", distinct)):
    got = {}
    for on in (False, True):
        eng.set_null_patterns(on)
        ms = []
        for i in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.null_intra_dev(kind, w["seed"] + 7, 0, nrep, ram, out["stat"], out["rcmin"], out["prmin"], out["nmin"], supplied=sup)
            b.record()
            torch.cuda.synchronize()
            if i:
                ms.append(a.elapsed_time(b))
        got[on] = {k: v.cpu().numpy().tobytes() for k, v in out.items()}
        res[f"{name}_{'patterns' if on else 'sites'}_ms"] = [round(x, 3) for x in ms]
        if on:
            res[f"{name}_patterns"] = eng.null_pattern_count()
            res[f"{name}_pattern_fraction"] = round(res[f"{name}_patterns"] / (2 * n), 5)
    res[f"{name}_same_bytes"] = all(got[False][k] == got[True][k] for k in got[True])
print(json.dumps(res))
