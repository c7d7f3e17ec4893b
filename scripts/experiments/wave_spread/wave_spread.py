#!/usr/bin/env python3
"""Per-wave busy time of the mapping kernel of a workload's null (a -DCMX_WAVE_SPREAD build of cmx_map.hip, see README.md here).
usage: COMAP_MI355X_LIB=build/abl/libcmx_spread.so python scripts/experiments/wave_spread/wave_spread.py target|cfg3|cfg4 [queue-off]

The null runs twice (the first run warms up); the probe keeps the last map_kernel launch: per wave its first and last
s_memtime, the site blocks it mapped and its workgroup.  Busy = last - first.  The launch lasts as long as its busiest wave,
so (max - mean) / max of the busy times is the share of the launch in which the average wave has nothing to do."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
import torch
import bench
from comap_amd import engine as E
from comap_amd.pipeline import IntraAnalysis

wl = sys.argv[1] if len(sys.argv) > 1 else "target"
lib = E.load_library()
if len(sys.argv) > 2 and sys.argv[2] == "queue-off":
    lib.cmx_debug_map_queue(ctypes.c_int(0))
w = bench.WORKLOADS[wl]
parent, blen, lot, mdl, Bk, clamp = bench.build_inputs(w)
eng = E.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk=Bk, clamp_negative=clamp)
dev = torch.device("cuda", 0)
aln_h, _ = eng.simulate(w["seed"] + 1, 0, w["nsites"])
ana = IntraAnalysis(eng, torch.from_numpy(aln_h).to(dev), w["statistic"], w["nclasses"])
nrep = w["nrep"](1)
ms = 0.0
for _ in range(2):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ana.null_distribution(w["seed"] + 7, 0, nrep, w["rep_ram"], map_events=(e0, e1))
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
buf = np.zeros((4096, 4), dtype=np.uint64)
assert lib.cmx_debug_read_wave_spread(buf.ctypes.data_as(ctypes.c_void_p)) == 0
b = buf[buf[:, 1] > 0].astype(np.float64)
t0, t1, nb, wg = b[:, 0], b[:, 1], b[:, 2], b[:, 3].astype(np.int64)
busy = t1 - t0
span = t1.max() - t0.min()   # (counters of different dies need not agree: the per-die figures below do not mix them)
pc = np.percentile(busy, [1, 50, 99])
print(f"{wl} null: map stage {ms:.3f} ms (events around pattern sort + mapping kernel + pair scoring), {len(b)} waves, {int(nb.sum())} blocks")
print(f"busy per wave (counts): mean {busy.mean():.4e} max {busy.max():.4e} min {busy.min():.4e}  p1 {pc[0]:.4e} p50 {pc[1]:.4e} p99 {pc[2]:.4e}")
print(f"(max - mean) / max = {100 * (busy.max() - busy.mean()) / busy.max():.2f} %   max / mean = {busy.max() / busy.mean():.4f}"
      f"   one block = {100 * busy.mean() / nb.mean() / busy.max():.2f} % of the busiest wave")
print(f"blocks per wave: min {int(nb.min())} max {int(nb.max())}; the busiest wave took {int(nb[busy.argmax()])}, the laziest {int(nb[busy.argmin()])};"
      f" per-block time of a wave: p1 {np.percentile(busy / nb, 1):.4e} p50 {np.percentile(busy / nb, 50):.4e} p99 {np.percentile(busy / nb, 99):.4e}")
print(f"start times: spread {t0.max() - t0.min():.3e} counts = {100 * (t0.max() - t0.min()) / busy.max():.3f} % of the busiest wave; first start to last end {span:.4e}")
print("by workgroup id mod 8 (accelerator die):  waves  mean busy  max busy  mean / overall mean  start spread  blocks")
for d in range(8):
    s = wg % 8 == d
    if s.any():
        print(f"  {d}: {int(s.sum()):5d}  {busy[s].mean():.4e}  {busy[s].max():.4e}  {busy[s].mean() / busy.mean():.4f}  {t0[s].max() - t0[s].min():.3e}  {int(nb[s].sum())}")
