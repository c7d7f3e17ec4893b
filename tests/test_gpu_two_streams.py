"""-m gpu: what runs on a second stream beside the null equals what runs alone.

The integrator's observed stage (mapping of the observed alignment, its Gram blocks, ancestral states) runs on a side
stream while the null distribution runs on the main one (bench.py).  Every observed stage is run here
against every kind of null, for a 20-state and a 4-state model, in the pattern of
test_variant_mapping_on_a_side_stream_beside_the_null (tests/test_gpu_parity.py): run(overlap=False) is the serial
reference, run(overlap=True) puts the observed stage on a torch.cuda.Stream with wait_stream both ways, three
overlapped runs, and every output of both sides must be equal with np.array_equal(.., equal_nan=True).

Every run is preceded, on the same context, by one host-path map_sites(aln, masks=...), so the context already records
that the leaf operators' ambiguity rows were built from a caller's table when the null starts (the host path
synchronises, so this part is deterministic).  The cells "mapping with a mask table" x "unfused null" are the ones
ADVICE.md (round 4) is about: the unfused null's own mapping used to rebuild the default rows on the null's stream
while the observed mapping of ambiguous codes was reading the caller's rows on the other.

Mapping options are one setting of the context and hold for both sides: in the seven cells of the observed stage
"map_noavg" the null runs unfused whatever the cell's null is called (fused_sites, fused_patterns and continuous there
repeat unfused_noavg with other settings and are no fused-null coverage); likewise every observed mapping beside
"unfused_noavg" is the nijt.average = no mapping.

Size of the observed alignment: its mapping has to be still in flight when the null's first kernels are enqueued.
README.md reports 3.9 ms for the observed stage of 10 000 x 64 protein sites; 4 000 sites on 48 taxa are a millisecond
or two of mapping, against some tens of microseconds between the two enqueues.

This module must not run under the scratch guard: with CMX_SCRATCH_GUARD on, every scratch() request calls
hipDeviceSynchronize() (comap_amd/csrc/cmx_api_ctx.cpp, scratch()) and the two streams never overlap.  The module fixture
switches the guard off for contexts it creates and puts the previous state back."""
import numpy as np
import pytest

import oracle
from comap_amd import engine, synthetic
from conftest import make_case

pytestmark = pytest.mark.gpu

NTAXA, NSITES = 48, 4000
NREP, RAM = 3, 200
ROWS = (0, 500)                       # rows of the pair loop whose Gram blocks are prefetched beside the null
BOUNDS = np.array([0.0, 1e-4, 1e-3, 1e-3, 0.01, 0.05, 0.3, 1.0, 50.0, 1e4])
OBSERVED = ["map", "map_masks", "map_prefetch", "asr_masks", "map_noavg"]
NULLS = ["fused_sites", "fused_patterns", "unfused_weights", "unfused_bounds", "unfused_noavg", "continuous", "inter"]


@pytest.fixture(scope="module", params=[20, 4], ids=["protein", "dna"])
def setup(request):
    import torch
    S = request.param
    was = engine.scratch_guard(False)
    case = make_case(NTAXA, NSITES, S, 4100 + S)
    rng = np.random.default_rng(S)
    if S == 4:
        masks = np.array([1, 2, 4, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15, 15], dtype=np.uint32)   # IUPAC + gap
        ncodes = 12
    else:
        masks = oracle.default_masks(20)[:24].copy()
        masks[20], masks[21] = (1 << 2) | (1 << 3), (1 << 5) | (1 << 6)                                # B, Z, X, gap
        ncodes = 4
    aln_amb = case["aln"].copy()
    hit = rng.random(aln_amb.shape) < 0.15
    aln_amb[hit] = rng.integers(S, S + ncodes, size=int(hit.sum()), dtype=np.uint8)
    table = np.full(256, (1 << S) - 1, dtype=np.uint32)          # the device entry points take the table padded to 256
    table[:len(masks)] = masks
    c2 = dict(case)
    c2["blen"] = case["blen"] * rng.uniform(0.5, 1.5, size=len(case["blen"]))
    m2 = synthetic.protein_model(0.9, 3) if S == 20 else synthetic.dna_model(0.9, 3)
    c2.update(rates=m2["rates"], probs=m2["probs"])
    mk = lambda c: engine.Engine(c["parent"], c["blen"], c["lot"], c["Q"], c["pi"], c["rates"], c["probs"])
    eng, eng2 = mk(case), mk(c2)
    dev = torch.device("cuda:0")
    st = dict(S=S, eng=eng, eng2=eng2, dev=dev, masks=masks, host_amb=np.ascontiguousarray(aln_amb[:, :50]),
              d_aln=torch.from_numpy(case["aln"]).to(dev), d_amb=torch.from_numpy(aln_amb).to(dev),
              d_masks=torch.from_numpy(table.view(np.int32)).to(dev), w=rng.uniform(0.2, 2.0, size=eng.B))
    yield st
    eng.close()
    eng2.close()
    engine.scratch_guard(was)


def _observed_stage(st, which):
    """-> (enqueue(): the part that runs beside the null, finish(): what follows once both streams have joined, outputs)"""
    import torch
    eng, dev, n = st["eng"], st["dev"], NSITES
    f64 = dict(dtype=torch.float64, device=dev)
    if which == "asr_masks":
        n_inner = len(eng.inner_nodes())
        states = torch.zeros(n_inner, n, dtype=torch.uint8, device=dev)
        post = torch.zeros(n_inner, eng.S, n, **f64)
        return (lambda: eng.ancestral_states_dev(st["d_amb"], states, post=post, masks=st["d_masks"])), (lambda: None), [states, post]
    out = dict(counts=torch.zeros(eng.B * eng.K, n, **f64), logL=torch.zeros(n, **f64), post_rate=torch.zeros(n, **f64),
               rate_class=torch.zeros(n, dtype=torch.int32, device=dev), norm=torch.zeros(n, **f64))
    if which == "map_masks":
        return (lambda: eng.map_sites_dev(st["d_amb"], masks=st["d_masks"], **out)), (lambda: None), list(out.values())
    if which in ("map", "map_noavg"):
        return (lambda: eng.map_sites_dev(st["d_aln"], **out)), (lambda: None), list(out.values())
    assert which == "map_prefetch"
    from comap_amd.pipeline import sum_pairs
    rec = torch.zeros(sum_pairs(n, *ROWS) * engine.PAIR_COMPACT.itemsize, dtype=torch.uint8, device=dev)

    def enqueue():
        eng.map_sites_dev(st["d_aln"], **out)
        eng.intra_gram_prefetch_dev(engine.STAT_CORRELATION, out["counts"], n, *ROWS)

    def finish():
        eng.intra_compact_range_dev(engine.STAT_CORRELATION, out["counts"], out["norm"], None, None, 4, rec, *ROWS)

    return enqueue, finish, list(out.values()) + [rec]


def _null(st, which):
    import torch
    eng, dev = st["eng"], st["dev"]
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(stat=torch.zeros(NREP * RAM, **f64), rcmin=torch.zeros(NREP * RAM, dtype=torch.int32, device=dev),
               prmin=torch.zeros(NREP * RAM, **f64), nmin=torch.zeros(NREP * RAM, **f64))
    if which == "unfused_bounds":
        run = lambda: eng.null_intra_dev(engine.STAT_DISCRETE_MI_BOUNDS, 9, 0, NREP, RAM, threshold=BOUNDS, **out)
    elif which == "continuous":
        run = lambda: eng.null_intra_continuous_dev(engine.STAT_CORRELATION, 9, 0, NREP, RAM, 0.7, p_invariant=0.1, **out)
    elif which == "inter":
        run = lambda: eng.null_inter_dev(st["eng2"], engine.STAT_CORRELATION, 9, 0, NREP, RAM, **out)
    else:
        run = lambda: eng.null_intra_dev(engine.STAT_CORRELATION, 9, 0, NREP, RAM, **out)
    return run, list(out.values())


def _settings(st, observed, null):
    eng = st["eng"]
    eng.set_null_patterns({"fused_sites": False, "fused_patterns": True}.get(null))
    eng.set_statistic_weights(st["w"] if null == "unfused_weights" else None)
    noavg = observed == "map_noavg" or null == "unfused_noavg"      # one setting of the context: it holds for both sides
    eng.set_mapping_options(not noavg, True)


@pytest.mark.parametrize("null", NULLS)
@pytest.mark.parametrize("observed", OBSERVED)
def test_observed_stage_beside_the_null(setup, observed, null):
    import torch
    st = setup
    eng, dev = st["eng"], st["dev"]

    def run(overlap):
        eng.map_sites(st["host_amb"], masks=st["masks"])          # the context's history: a caller's mask table
        enqueue, finish, obs_out = _observed_stage(st, observed)
        null_run, null_out = _null(st, null)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        if overlap:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                enqueue()
            null_run()
            torch.cuda.current_stream().wait_stream(side)
        else:
            enqueue()
            torch.cuda.synchronize()
            null_run()
        finish()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in obs_out + null_out]

    _settings(st, observed, null)
    try:
        seq = run(False)
        assert np.isfinite(seq[-4]).any()                         # the null scored something
        for k in range(3):
            ovl = run(True)
            for i, (a, b) in enumerate(zip(seq, ovl)):
                assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), \
                    "overlapped run %d: output %d of (%s beside %s) differs from the serial run" % (k, i, observed, null)
    finally:
        eng.set_null_patterns(None)
        eng.set_statistic_weights(None)
        eng.set_mapping_options(True, True)
