#!/usr/bin/env python3
"""Benchmark of the substitution-mapping + pairwise-coevolution hot path on MI355X.

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch of synthetic input (DESIGN.md section "Measurement"):
  map the observed alignment  ||  parametric-bootstrap null for this rank's replicates (simulate, re-map twice, score)
  -> [N > 1: one RCCL all-gather of the null] -> all-pairs statistic on MFMA + p-values for this rank's row block
Metric (BASELINE.json): site-pair coevolution statistics/s incl. null sims = (observed pairs + null pairs) / time,
inputs resident in HBM when the timed region starts.

Default workload = the configuration the metric is quoted on (BASELINE.json north_star): 10 000-column x 64-taxa
protein alignment, JTT92+G4, correlation, 1 000 null replicates x 10 000 sites.  With N GPUs the SAME 1 000
replicates are sharded over the ranks (strong scaling) and the observed all-pairs stage is split in row blocks.
A plain run sets up, warms up, times the steps and prints the headline.  With --full the JSON line also carries:
`roofline` (dominant kernel, HIP events on its stream), `cpu_baseline`
(oracle on the host cores, 1 thread as the reference runs + all cores), `host_to_host` (same step with the alignment
coming from and the statistics / p-values going to host memory: BASELINE.md section 3's counting rule) and
`mica_cfg5` (BASELINE configs[4], the Mica column-MI kernel with its own roofline and CPU figure); --no-cpu-baseline,
--no-host and --no-mica leave one of them out.
--dump-outputs DIR writes what the last timed step handed its caller to DIR/<name>.npy (float64; see dump_outputs).
"""
import argparse
import glob
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: ntaxa, nsites, nstates, tree seed, statistic, total null replicates at N GPUs, rep_ram, norm classes
    "target": dict(ntaxa=64, nsites=10000, nstates=20, seed=20260101, statistic="Correlation", nrep=lambda n: 1000,
                   rep_ram=10000, nclasses=10, scaling="strong",
                   desc="north-star target: 10000x64 protein JTT92+G4(a=0.5), correlation, 1000 null replicates x 10000"),
    "cfg2": dict(ntaxa=64, nsites=2000, nstates=20, seed=20260101, statistic="Correlation", nrep=lambda n: 0,
                 rep_ram=2000, nclasses=10, scaling="strong",
                 desc="BASELINE configs[1]: 2000x64 protein JTT92+G4(a=0.5), correlation, no null (map + all pairs + rows)"),
    "cfg3": dict(ntaxa=64, nsites=2000, nstates=20, seed=20260101, statistic="Correlation", nrep=lambda n: 125 * n,
                 rep_ram=2000, nclasses=10, scaling="weak",
                 desc="2000x64 protein JTT92+G4(a=0.5), correlation, null 125 rep/GPU x 2000 (configs[2] at 8 GPUs)"),
    "cfg4": dict(ntaxa=256, nsites=10000, nstates=4, seed=20260102, statistic="Compensation", nrep=lambda n: 12 * n,
                 rep_ram=10000, nclasses=10, scaling="weak",
                 desc="10000x256 DNA GTR+G4, compensation (W=idx[y]-idx[x]), null 12 rep/GPU x 10000"),
}
FP64_PEAK_TFLOPS = 78.6   # MI355X public spec, vector == matrix fp64 (the microarch guide has no fp64 row);
# measured here (scripts/ubench_f64.hip): v_mfma_f64_16x16x4 72-75, v_mfma_f64_4x4x4_4b 65-68, v_fma_f64 55-59 TFLOP/s
HBM_PEAK_TBPS = 8.0       # guide, HBM: 8.0 TB/s spec (6.3 TB/s measured with a streaming copy)
INT8_PEAK_TOPS = 5000.0   # guide, Matrix cores: I8 = 2x the BF16 rate per clock, BF16 ~2.5 PF dense


def build_inputs(w):
    from comap_amd import synthetic as sy
    parent, blen, lot = sy.random_tree(w["ntaxa"], w["seed"])
    if w["nstates"] == 20:
        mdl = sy.protein_model(0.5, 4)
        Bk, clamp = None, True
    else:
        mdl = sy.dna_model(0.5, 4)
        Bk = sy.weighted_register(mdl["Q"], sy.compensation_weights_dna())[None] if w["statistic"] == "Compensation" else None
        clamp = Bk is None
    return parent, blen, lot, mdl, Bk, clamp


def flops_per_site(info, B, C, S, K, null=False):
    """algorithmic: SURVEY 8(d), F_map = 7 B C S^2 (K = 1) -- every branch, leaf branches included, priced as dense
    products.  executed: what the kernel issues on the matrix cores (info = cmx_get_info: products of one device-class
    pass over device states; leaf branches are row gathers, sibling messages are stored, not recomputed; null: the walk of
    the null's resolved alignments, where class-fused nucleotide models take cherries from tables)."""
    algorithmic = 7.0 * B * C * S * S
    dS, dC = info["device_states"], info["device_classes"]
    fuse = max(1, dS // S)   # class-fused nucleotide model: block-diagonal operators, only the diagonal tiles are applied
    tables = null and info.get("cherry_tables", 0) > 0
    products = info["products_per_pass_null"] if tables else info["products_per_pass"]
    leaf_ops = info["leaf_ops_per_pass_null"] if tables else info["leaf_ops_per_pass"]
    executed = dC * (products * 2.0 * dS * dS / fuse + leaf_ops * 2.0 * dS)
    return algorithmic, executed


def kernel_source_sha():
    """sha of the device sources: a PMC traffic figure in profiles/ is attached only when it was taken on this code"""
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "comap_amd", "csrc", "*.hip")) +
                    glob.glob(os.path.join(ROOT, "comap_amd", "csrc", "*.h"))):
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def cpu_baseline(w, parent, blen, lot, mdl, Bk, clamp, nrep_total):
    """Oracle (CPU restatement, reference loop structure) on a bounded sample, extrapolated to the step's unit mix.
    kind = "port": the reference itself cannot be built here (Bio++ absent).  The headline figure is ONE thread, as the
    reference runs; `all_cores` repeats the dominant stage (the null) with one replicate range per host thread."""
    import concurrent.futures as cf
    import oracle
    kind = {"Correlation": 0, "Compensation": 1}[w["statistic"]]
    om = oracle.Model(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk=Bk, nonneg=clamp)
    n_obs = min(w["nsites"], 2000)
    nrep_s, ram_s = 16, min(w["rep_ram"], 2000)   # 64 000 sites re-mapped: 10-15 s on one core
    aln, _ = oracle.simulate(om, w["seed"] + 1, 0, n_obs)
    t0 = time.perf_counter()
    m = oracle.map_sites(om, aln)
    t_map = time.perf_counter() - t0
    t0 = time.perf_counter()
    st = oracle.pair_stats_intra(kind, m["counts"])
    t_pairs = time.perf_counter() - t0
    if nrep_total == 0:   # no null (BASELINE configs[1]): mapping + the pair loop is the whole job, nothing is extrapolated
        pairs = n_obs * (n_obs - 1) / 2
        return dict(value=pairs / (t_map + t_pairs), unit="site-pair statistics/s", cores=1, kind="port",
                    sample=f"oracle/oracle.c -O2, 1 thread, the whole workload: map {n_obs} sites {t_map:.2f}s + {int(pairs)} pair stats {t_pairs:.2f}s")
    t0 = time.perf_counter()
    nl = oracle.null_intra(om, kind, 1, 0, nrep_s, ram_s)
    t_null = time.perf_counter() - t0
    t0 = time.perf_counter()
    oracle.intra_pvalues(st, m["norm"], w["nclasses"], nl["stat"], nl["nmin"])
    t_pv = time.perf_counter() - t0
    scale_obs = w["nsites"] / n_obs
    pairs_obs = w["nsites"] * (w["nsites"] - 1) / 2
    null_pairs_total = nrep_total * w["rep_ram"]
    null_scale = null_pairs_total / (nrep_s * ram_s)

    def full_time(t_null_sample, div=1.0):
        return (t_map * scale_obs / div + t_pairs * scale_obs ** 2 / div + t_null_sample * null_scale
                + t_pv * scale_obs ** 2 * null_scale / div)   # linear-scan p-values scale with nsim
    t_full = full_time(t_null)
    # all host cores: the replicate loop (AnalysisTools.cpp:587) split over threads (the C oracle is re-entrant and
    # ctypes releases the GIL); the observed stages are divided by the thread count as perfectly parallel loops
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    nthr = max(1, min(cores, 64))
    nrep_mt = max(nrep_s, 2 * nthr)
    bounds = np.linspace(0, nrep_mt, nthr + 1).astype(int)
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(nthr) as ex:
        list(ex.map(lambda i: oracle.null_intra(om, kind, 1, int(bounds[i]), int(bounds[i + 1]), ram_s), range(nthr)))
    t_null_mt = (time.perf_counter() - t0) * nrep_s / nrep_mt
    t_full_mt = full_time(t_null_mt, div=nthr)
    unit = "site-pair statistics/s"
    sample = (f"oracle/oracle.c -O2, 1 thread: map {n_obs} sites {t_map:.2f}s, {n_obs * (n_obs - 1) // 2} pair stats "
              f"{t_pairs:.2f}s, null {nrep_s} rep x {ram_s} (={2 * nrep_s * ram_s} sites re-mapped) {t_null:.2f}s, "
              f"linear-scan p-values {t_pv:.2f}s; extrapolated to the step's unit mix ({t_full:.0f}s of CPU work)")
    return dict(value=(pairs_obs + null_pairs_total) / t_full, unit=unit, cores=1, kind="port", sample=sample,
                all_cores=dict(value=(pairs_obs + null_pairs_total) / t_full_mt, unit=unit, cores=nthr,
                               sample=f"null {nrep_mt} rep x {ram_s} over {nthr} threads (one replicate range each) "
                                      f"{t_null_mt * nrep_mt / nrep_s:.2f}s; observed stages / {nthr}; extrapolated "
                                      f"({t_full_mt:.0f}s)"))


def mica_leg(dev, steps, world=1, rank=0, gloo=False):
    """BASELINE configs[4]: Mica column MI of 5000 + 5000 columns, 256 taxa, protein alphabet, all 25e6 cross pairs
    (Mica.cpp:349-361, 646-689), inputs resident in HBM.  With N ranks the rectangle is split by rows of the first
    alignment and ONE all-reduce of the column sums gives the averages of APC / RCW (comap_amd.distributed.mica_rectangle).
    Own roofline (one-hot Gram, 2 A^2 T int8 ops per pair) and, at N = 1, own CPU figure (oracle's SiteTools restatement on
    a 300 x 300 column sample)."""
    import torch
    import torch.distributed as dist
    from comap_amd import engine as E
    from comap_amd.distributed import mica_rectangle
    rng = np.random.default_rng(20260103)
    T, A, n1, n2 = 256, 20, 5000, 5000
    base = rng.integers(0, A, size=(T, 1))
    a1 = np.where(rng.random((T, n1)) < 0.6, base, rng.integers(0, A, size=(T, n1))).astype(np.uint8)
    a2 = np.where(rng.random((T, n2)) < 0.4, base, rng.integers(0, A, size=(T, n2))).astype(np.uint8)
    d1, d2 = torch.from_numpy(a1).to(dev), torch.from_numpy(a2).to(dev)
    eng = E.Engine(device=dev.index)
    r = mica_rectangle(eng, d1, d2, A)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = mica_rectangle(eng, d1, d2, A)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    el = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([el], dtype=torch.float64, device=torch.device("cpu") if gloo else dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        el = float(tt.item())
    ms = 1e3 * el / steps
    pairs = n1 * n2
    b, e = r["rows"]
    ident = float((r["mi"] - (r["h1"][:, None] + r["h2"][None, :] - r["hjoint"])).abs().max())
    tops = pairs * 2.0 * A * A * T / (ms * 1e-3) / 1e12
    out = dict(workload="cfg5: Mica MI, 5000 + 5000 columns x 256 taxa, protein alphabet, all 25e6 cross pairs",
               value=pairs / (ms * 1e-3), unit="column-pair MI/s", ms_per_step=ms, steps=steps, dtype="i8", n_gpus=world,
               parallelism=("single GPU" if world == 1 else f"rows of alignment 1 split x{world}, one all-reduce of the column sums"),
               roofline=dict(bound="mfma", kernel="mica_mfma4_kernel<8, plain> (+ symbol bytes / column sums / row and column means)", achieved=tops,
                             peak=INT8_PEAK_TOPS * world, unit="TOP/s", frac=tops / (INT8_PEAK_TOPS * world), traffic=None,
                             ops_per_pair_algorithmic=2.0 * A * A * T),
               max_identity_residual=ident, full_mean_mi=float(r["full_mean"]))
    # HBM bytes per call of the dominant kernel from the PMC passes, only if they were taken on these device sources
    for tf in sorted(glob.glob(os.path.join(ROOT, "profiles", "traffic_r*.json")), reverse=True):
        try:
            t = json.load(open(tf))
            if t.get("kernel_source_sha") == kernel_source_sha() and "mica_cfg5" in t:
                out["roofline"]["traffic"] = t["mica_cfg5"] / world
                out["roofline"]["traffic_source"] = os.path.relpath(tf, ROOT)
                break
        except Exception:
            pass
    if world == 1:
        import oracle
        ns = 300
        t0 = time.perf_counter()
        o = oracle.mi_columns(a1[:, :ns], a2[:, :ns], A)
        t_cpu = time.perf_counter() - t0
        out["cpu_baseline"] = dict(value=ns * ns / t_cpu, unit="column-pair MI/s", cores=1, kind="port",
                                   sample=f"oracle/oracle.c orc_mi_columns on {ns} x {ns} columns: {t_cpu:.2f}s")
        out["max_abs_diff_vs_oracle_sample"] = float(np.max(np.abs(o["mi"] - r["mi"][:ns, :ns].cpu().numpy())))
    eng.close()
    return out


DUMP_SAMPLE = 1 << 19        # entries kept of a larger output: 4 MB per array, the whole dump well under DUMP_MAX_BYTES
DUMP_MAX_BYTES = 64 << 20


def _sample(n, k, seed):
    """sorted positions of a fixed, seeded sample of k of n entries (all of them when n <= k)"""
    if n <= k:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.default_rng(seed).choice(n, k, replace=False))


def dump_outputs(out_dir, ana, last, pair_output, row_begin, row_end, n_null, suffix=""):
    """--dump-outputs: what the last timed step handed its caller, as float64 <out_dir>/<name><suffix>.npy -- the
    observed mapping (per-site vectors; `counts` on a sample of sites, `counts_sites`), this rank's null (`null_*`, at
    positions `null_pos`) and this rank's pairs in the --pair-output form (`pair_*`, pair (pair_i, pair_j)).  An output of
    more than DUMP_SAMPLE entries is a fixed, seeded sample, so two builds' dumps compare entry for entry."""
    import torch
    from comap_amd import engine as E
    dev = ana.aln.device
    n = ana.n

    def take(t, pos):
        return t.reshape(-1)[torch.from_numpy(pos).to(dev)]

    arrays = dict(norm=ana.norm, post_rate=ana.post_rate, rate_class=ana.rate_class, logL=ana.logL)
    sites = _sample(n, max(1, DUMP_SAMPLE // ana.counts.shape[0]), 1)
    arrays["counts"] = ana.counts[:, torch.from_numpy(sites).to(dev)]
    arrays["counts_sites"] = sites
    if n_null:
        b = ana.null_buffers(n_null)
        pos = _sample(n_null, DUMP_SAMPLE, 2)
        arrays.update(null_stat=take(b["stat"], pos), null_nmin=take(b["nmin"], pos), null_pos=pos)
    if pair_output == "dense":
        pos = _sample(n * n, DUMP_SAMPLE, 3)
        arrays.update(pair_i=pos // n, pair_j=pos % n, pair_stat=take(ana.stat, pos), pair_pvalue=take(ana.pvalue, pos),
                      pair_nsim=take(ana.nsim, pos))
    else:
        buf, count = last
        dt = E.PAIR_COMPACT if pair_output == "compact" else E.PAIR_ROW
        npairs = count if pair_output == "compact" else int(count.item())
        pos = _sample(npairs, DUMP_SAMPLE, 3)
        rec = buf[:npairs * dt.itemsize].view(npairs, dt.itemsize)[torch.from_numpy(pos).to(dev)]
        rec = rec.cpu().numpy().view(dt).ravel()
        if pair_output == "compact":   # records in (i, j) order over rows [row_begin, row_end): row i starts at off[i - row_begin]
            r = np.arange(row_begin, row_end + 1, dtype=np.int64)
            off = (r - row_begin) * (n - 1) - (r * (r - 1) - row_begin * (row_begin - 1)) // 2
            i = row_begin + np.searchsorted(off, pos, side="right") - 1
            arrays.update(pair_i=i, pair_j=i + 1 + pos - off[i - row_begin])
        arrays.update({"pair_" + f: rec[f] for f in dt.names})
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: (v.cpu().numpy() if torch.is_tensor(v) else v).astype(np.float64) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_MAX_BYTES, total
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + suffix + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)   # 10 x 0.47 s: one slow step (a busy host core) weighs a tenth
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="target", choices=sorted(WORKLOADS))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-mica", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--pair-output", default="compact", choices=["compact", "rows", "dense"],
                    help="observed pair loop of this rank's row range: 16-byte records per pair (statistic, null count, class size; default -- "
                         "the job has no pair filters, cmx_expand_compact_rows rebuilds the 48-byte rows on the host), the 48-byte "
                         "statistics.txt rows compacted on the device, or dense N x N matrices")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also the roofline, host-to-host, CPU baseline and Mica legs (runs of their own)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (float64, a seeded sample of large outputs)")
    args = ap.parse_args()

    import torch
    import torch.distributed as dist
    from comap_amd import engine as E
    from comap_amd.pipeline import IntraAnalysis

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    # rehearsal on a one-GPU box (CMX_BENCH_REHEARSAL=1): all ranks share device 0 and the exchange runs over gloo;
    # it checks the N > 1 control flow only, its throughput means nothing
    rehearsal = os.environ.get("CMX_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    w = WORKLOADS[args.workload]
    parent, blen, lot, mdl, Bk, clamp = build_inputs(w)
    eng = E.Engine(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], Bk=Bk, clamp_negative=clamp,
                   device=local_rank)
    info = eng.info()
    # observed alignment: simulated by the engine's own simulator (seed + 1), resident in HBM before timing starts
    aln_h, _ = eng.simulate(w["seed"] + 1, 0, w["nsites"])
    d_aln = torch.from_numpy(aln_h).to(dev)
    ana = IntraAnalysis(eng, d_aln, w["statistic"], w["nclasses"])
    from comap_amd.distributed import gather_null, replicate_shard, row_shard
    from comap_amd.pipeline import sum_pairs
    ram = w["rep_ram"]
    nrep_total = w["nrep"](world)
    rep_begin, rep_end = replicate_shard(rank, world, nrep_total)
    n_local = (rep_end - rep_begin) * ram
    row_begin, row_end = row_shard(rank, world, w["nsites"])   # this rank's share of the observed pair loop
    # recorded in every timed step, --full or not: with them the null is simulated and mapped in two launches
    # (IntraAnalysis.null_distribution), the timed path the headline has always measured
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(args.steps)]
    ev_sim = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(args.steps)]
    side = torch.cuda.Stream(device=dev)   # observed-alignment mapping overlaps the null kernel (independent work)
    main_s = torch.cuda.current_stream()

    def step(i, timed, aln=None):
        if nrep_total == 0:   # no null: map, then the pair loop without p-values; the events bracket the mapping stage
            if timed:
                ev[i][0].record()
            ana.get_vectors(aln)
            if timed:
                ev[i][1].record()
            if args.pair_output == "compact":
                return ana.compute_intra_compact(None, None, row_begin, row_end)
            if args.pair_output == "rows":
                return ana.compute_intra_rows(None, None, row_begin, row_end)
            ana.compute_intra_stats(None, None)
            return None
        side.wait_stream(main_s)
        with torch.cuda.stream(side):
            ana.get_vectors(aln)
            if args.pair_output == "compact":   # the observed pairs' statistics too: they do not wait for the null
                ana.prefetch_intra_gram(row_begin, row_end)
        # the null: simulate (own kernel, full occupancy) then map + score; the events bracket the mapping launch alone
        nb = ana.null_distribution(w["seed"] + 7, rep_begin, rep_end, ram, map_events=ev[i] if timed else None,
                                   sim_events=ev_sim[i] if timed else None)
        main_s.wait_stream(side)
        # the path's one exchange: every rank needs the merged null before p-values (one RCCL all-gather)
        ns, nm = gather_null(nb["stat"], nb["nmin"], nrep_total, ram)
        if args.pair_output == "compact":   # statistic + null count of every pair of this rank's rows, 16 B per pair, (i, j) order
            return ana.compute_intra_compact(ns, nm, row_begin, row_end)
        if args.pair_output == "rows":   # statistic + p-value + filters + compaction for this rank's rows, no N x N matrix
            return ana.compute_intra_rows(ns, nm, row_begin, row_end)
        ana.compute_intra_stats(ns, nm)    # dense N x N statistic / p-value / Nsim (every rank, all pairs)
        return None

    for i in range(args.warmup):
        step(i, False)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        last = step(i, True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=torch.device("cpu") if rehearsal else dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    pairs_obs = w["nsites"] * (w["nsites"] - 1) // 2
    units_per_step = pairs_obs + nrep_total * ram
    ms_per_step = 1e3 * elapsed / args.steps
    value = units_per_step * args.steps / elapsed

    out = dict(metric="site-pair coevolution statistics/s (incl. null sims)", value=value,
               unit="site-pair statistics/s", n_gpus=world, steps=args.steps, warmup=args.warmup,
               ms_per_step=ms_per_step, higher_is_better=True, scaling=w["scaling"], vs_baseline=None, dtype="f64",
               data="synthetic",
               config=dict(workload=f"{args.workload}: {w['desc']}", observed_pairs=pairs_obs,
                           null_pairs_total=nrep_total * ram, null_pairs_this_gpu=n_local,
                           sites_mapped_per_step_this_gpu=w["nsites"] + 2 * n_local,
                           parallelism=(f"null replicates and observed row blocks sharded x{world}, one RCCL all-gather" if world > 1 else "single GPU"),
                           pair_output=args.pair_output, observed_rows_this_gpu=[row_begin, row_end],
                           cu_count=info["cu_count"], mapping_waves=info["waves"],
                           walk_per_pass=dict(products=info["products_per_pass"], leaf_ops=info["leaf_ops_per_pass"],
                                              ws_loads=info["ws_loads_per_pass"], ws_stores=info["ws_stores_per_pass"],
                                              cherry_tables=info["cherry_tables"], products_null=info["products_per_pass_null"],
                                              leaf_ops_null=info["leaf_ops_per_pass_null"])))
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, ana, last, args.pair_output, row_begin, row_end, n_local,
                     f".rank{rank}" if world > 1 else "")

    if args.full:
        # roofline of the dominant kernel (map_kernel<S, null>): HIP events on the launch stream
        null_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
        alg, exe = flops_per_site(info, eng.B, eng.C, eng.S, eng.K, null=nrep_total > 0)
        sites_per_launch = 2 * n_local if nrep_total else w["nsites"]
        achieved = sites_per_launch * alg / (null_ms * 1e-3) / 1e12
        ach_exe = sites_per_launch * exe / (null_ms * 1e-3) / 1e12
        # `achieved` / `frac` follow SURVEY 8(d): ALGORITHMIC flops (7 B C S^2 per site, leaf edges counted as dense
        # products) / time / peak.  `frac_executed` counts only the matrix products the kernel issues (leaf edges are row
        # gathers, sibling messages are stored instead of recomputed): the matrix pipe's duty, always lower.
        sim_ms = float(np.mean([a.elapsed_time(b) for a, b in ev_sim])) if nrep_total else 0.0
        kname = f"map_kernel<{eng.S},null>" if nrep_total else f"map_kernel<{eng.S},observed> (+ map_finalize_kernel when class-split)"
        roofline = dict(bound="mfma", kernel=kname, achieved=achieved, peak=FP64_PEAK_TFLOPS,
                        unit="TFLOP/s", frac=achieved / FP64_PEAK_TFLOPS, traffic=None,
                        launch_ms=null_ms, simulate_ms=sim_ms, sites_per_launch=sites_per_launch, flops_per_site_algorithmic=alg,
                        flops_per_site_executed=exe, achieved_executed=ach_exe, frac_executed=ach_exe / FP64_PEAK_TFLOPS)
        # what is left of a step besides the simulator and the null's mapping launch: at N = 1 the observed stage (null sort +
        # index, Gram, p-value lookup, filters, compacted rows; the observed alignment's mapping runs beside the null); at N > 1
        # the all-gather too
        roofline["rest_of_step_ms"] = ms_per_step - null_ms - sim_ms
        if nrep_total:
            # In the timed steps the observed alignment's mapping and the observed pairs' Gram run on the side stream beside this
            # launch and share its CUs (they cost a protein null nothing measurable, the short nucleotide null of cfg4 up to a
            # tenth).  Outside the timed region: the same launch with nothing beside it -- the kernel's own figure.
            roofline["concurrent_in_timed_steps"] = "observed mapping + observed pairs' Gram (side stream)"
            torch.cuda.synchronize()
            ev_alone = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(2)]
            for e2 in ev_alone:
                ana.null_distribution(w["seed"] + 7, rep_begin, rep_end, ram, map_events=e2)
            torch.cuda.synchronize()
            alone_ms = float(np.mean([a.elapsed_time(b) for a, b in ev_alone]))
            roofline["launch_ms_alone"] = alone_ms
            roofline["frac_alone"] = sites_per_launch * alg / (alone_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS
        for tf in sorted(glob.glob(os.path.join(ROOT, "profiles", "traffic_r*.json")), reverse=True):
            try:
                t = json.load(open(tf))
                if t.get("kernel_source_sha") == kernel_source_sha() and args.workload in t:
                    # per-launch bytes measured at N = 1; a sharded launch maps fewer sites (the traffic is per-site state)
                    ref_sites = t.get("sites_per_launch", {}).get(args.workload, sites_per_launch)
                    roofline["traffic"] = t[args.workload] * sites_per_launch / ref_sites
                    roofline["traffic_source"] = os.path.relpath(tf, ROOT)
                    break
            except Exception:
                pass
        # next to the contract's algorithmic figure, say which roof the kernel really sits nearer to -- the fraction
        # of the fp64 pipe it keeps busy (executed flops) against the fraction of the HBM rate its measured bytes take
        if roofline["traffic"] is not None:
            hbm_tbs = roofline["traffic"] / (null_ms * 1e-3) / 1e12
            roofline["hbm_achieved_TBps"] = hbm_tbs
            roofline["hbm_frac"] = hbm_tbs / HBM_PEAK_TBPS
            roofline["nearest_roof"] = ("hbm" if roofline["hbm_frac"] > roofline["frac_executed"] else "fp64")
            # VERDICT r3 / ADVICE r3: the label follows the measured nearer roof; achieved / peak / frac stay SURVEY 8(d)'s
            # algorithmic fp64 figure (the contract's figure), the HBM side is hbm_achieved_TBps / hbm_frac
            roofline["bound"] = "hbm" if roofline["nearest_roof"] == "hbm" else "mfma"
            roofline["note"] = ("bound / achieved / frac price the ALGORITHMIC flops of SURVEY 8(d) (leaf edges as dense products); the kernel "
                                "executes frac_executed of the fp64 peak in matrix products and moves `traffic` bytes = hbm_frac of the 8 TB/s "
                                "HBM spec (its per-site intermediate state and the operator stream, DESIGN.md 4.1)")
        out["roofline"] = roofline

    # same step, host memory to host memory (SURVEY 8(d) / BASELINE.md section 3: the contract's clock; never `value`): the
    # alignment is uploaded inside the timed region and the statistic + p-value information of every pair ends in (pinned)
    # host memory.  Same --steps / --warmup as the headline.
    if args.full and not args.no_host and world == 1:
        h_aln = torch.from_numpy(aln_h).pin_memory()
        d_in = torch.empty_like(d_aln)
        npairs_rank = sum_pairs(w["nsites"], row_begin, row_end)
        if args.pair_output == "compact":
            hs = [torch.empty(npairs_rank * E.PAIR_COMPACT.itemsize, dtype=torch.uint8, pin_memory=True)]
        elif args.pair_output == "rows":
            hs = [torch.empty(npairs_rank * E.PAIR_ROW.itemsize, dtype=torch.uint8, pin_memory=True)]
        else:
            hs = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (ana.stat, ana.pvalue, ana.nsim)]
        h_site = [torch.empty(w["nsites"], dtype=torch.float64, pin_memory=True) for _ in range(2)] + \
                 [torch.empty(w["nsites"], dtype=torch.int32, pin_memory=True)]

        def host_step(i):
            d_in.copy_(h_aln, non_blocking=True)
            out_rows = step(i, False, d_in)
            nbytes = 0
            if args.pair_output == "compact":
                nbytes = out_rows[1] * E.PAIR_COMPACT.itemsize
                hs[0][:nbytes].copy_(out_rows[0][:nbytes], non_blocking=True)
                # what cmx_expand_compact_rows needs besides the records: posterior rate, norm, rate class of every site
                for h, t in zip(h_site, (ana.post_rate, ana.norm, ana.rate_class)):
                    h.copy_(t, non_blocking=True)
                    nbytes += h.numel() * h.element_size()
            elif args.pair_output == "rows":
                nrows = int(out_rows[1].item())          # rows that passed the filters (all pairs by default)
                nbytes = nrows * E.PAIR_ROW.itemsize
                hs[0][:nbytes].copy_(out_rows[0][:nbytes], non_blocking=True)
            else:
                for h, t in zip(hs, (ana.stat, ana.pvalue, ana.nsim)):
                    h.copy_(t, non_blocking=True)
                    nbytes += h.numel() * h.element_size()
            torch.cuda.synchronize()
            return nbytes

        for i in range(args.warmup):
            host_step(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            d2h = host_step(0)
        th = (time.perf_counter() - t0) / args.steps
        notes = {"compact": "16 B per pair (Stat, null count, class size) + the per-site PRmin / Nmin / RCmin sources",
                 "rows": "compacted statistics.txt rows (48 B per pair: i, j, Stat, RCmin, PRmin, Nmin, PValue, Nsim)",
                 "dense": "dense statistic / p-value / Nsim"}
        out["host_to_host"] = dict(value=units_per_step / th, unit="site-pair statistics/s", ms_per_step=1e3 * th, steps=args.steps,
                                   warmup=args.warmup, h2d_bytes=int(h_aln.numel()), d2h_bytes=int(d2h),
                                   vs_resident=(units_per_step / th) / value,
                                   note="alignment H2D + " + notes[args.pair_output] + " D2H (pinned) inside the timed region")
        if args.pair_output == "compact":
            # the expansion to the reference's 48-byte rows is host work outside the contract's clock (like text formatting): timed once
            rec = hs[0][:npairs_rank * E.PAIR_COMPACT.itemsize].numpy().view(E.PAIR_COMPACT)
            nthr = min(16, os.cpu_count() or 1)
            t0 = time.perf_counter()
            rows_h = E.expand_compact_rows(w["nsites"], row_begin, row_end, h_site[2].numpy(), h_site[0].numpy(), h_site[1].numpy(), rec, nthr)
            out["host_to_host"]["expand_rows"] = dict(ms=1e3 * (time.perf_counter() - t0), threads=nthr, rows=int(len(rows_h)),
                                                      note="cmx_expand_compact_rows: 48-byte statistics.txt rows rebuilt on the host, outside the timed region")
            del rows_h, rec
        del hs, h_aln, d_in, h_site

    if args.full and rank == 0:
        if args.no_cpu_baseline or world > 1:   # CPU baseline: rank 0 at N = 1 only
            out["cpu_baseline"] = None
        else:
            out["cpu_baseline"] = cpu_baseline(w, parent, blen, lot, mdl, Bk, clamp, nrep_total)
    if args.full and not args.no_mica:
        del ana
        torch.cuda.empty_cache()
        out["mica_cfg5"] = mica_leg(dev, max(3, args.steps), world, rank, rehearsal)
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
