#!/usr/bin/env python3
"""Sliding-window p-values (cmx_window_null_dev, cmx_intra_window_range_dev) at bench.py's shapes: the index build, the record pass
of all pairs at window 0.02 and 0.2 (the pass must not grow with the window), and for scale the binned
cmx_intra_compact_range_dev call in the same process.  Every timed call finds its Gram blocks kept
(cmx_intra_gram_prefetch_dev, untimed), so neither side's time holds the pair statistics.  Device events, median of 7.
usage: python scripts/bench_window_pvalues.py [target cfg2 ...]   (GPU box, repo root)  -> one JSON line per workload"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

import bench
from comap_amd import engine as E
from comap_amd.pipeline import IntraAnalysis, sum_pairs

REPS = 7


def timed(run, before=None):
    ts = []
    for _ in range(REPS + 1):          # the first one warms up
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts = sorted(ts[1:])
    return dict(median_ms=ts[REPS // 2], min_ms=ts[0], max_ms=ts[-1])


def one(wl):
    w = bench.WORKLOADS[wl]
    parent, blen, lot, mdl, Bk, clamp = bench.build_inputs(w)
    eng = E.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk=Bk, clamp_negative=clamp)
    aln_h, _ = eng.simulate(w["seed"] + 1, 0, w["nsites"])
    ana = IntraAnalysis(eng, torch.from_numpy(aln_h).cuda(), w["statistic"], w["nclasses"])
    ana.get_vectors()
    nrep = max(w["nrep"](1), 125)      # cfg2 has no null of its own: cfg3's
    nb = ana.null_distribution(w["seed"] + 7, 0, nrep, w["rep_ram"])
    ns, nm = nb["stat"].clone(), nb["nmin"].clone()
    n = ana.n
    out = dict(workload=wl, nsites=n, pairs=sum_pairs(n, 0, n), nnull=int(ns.numel()), reps=REPS, timer="device events, median of 7")
    rec = torch.empty(out["pairs"] * E.PAIR_WINDOW.itemsize, dtype=torch.uint8, device="cuda")
    for window in (0.02, 0.2):
        out["index_build_w%g" % window] = timed(lambda: eng.window_null_dev(ns, nm, window))
        out["record_pass_w%g" % window] = timed(lambda: eng.intra_window_range_dev(ana.kind, ana.counts, ana.norm, rec), ana.prefetch_intra_gram)
        nobs = torch.from_numpy(rec.cpu().numpy().view(E.PAIR_WINDOW)["nobs"].astype("int64"))
        out["mean_nobs_w%g" % window] = float(nobs.double().mean())
    out["index"] = eng.window_null_info()
    out["binned_class_table_and_record_pass"] = timed(lambda: ana.compute_intra_compact(ns, nm), ana.prefetch_intra_gram)
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    for wl in sys.argv[1:] or ["target", "cfg2"]:
        one(wl)
