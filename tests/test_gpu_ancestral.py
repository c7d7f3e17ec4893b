"""asr.method = marginal (CoMap/CoMap.cpp:169-197, cmx_ancestral_states*) on the device against the oracle's marginal
states and posteriors (oracle.map_sites_marginal, pinned by tests/test_oracle_marginal.py) and, for non-homogeneous model
sets, the numpy restatement (tests/ancestral_reference.py).  Posteriors to 1e-9 absolute; states equal wherever the
oracle's margin (best - second) / best exceeds 1e-9, and at least 97 % of the (site, node) cells are that clear.
Then the exact-equality properties: pass boundaries, a side stream beside the null, independence of the mapping options
and weights, no effect on a later mapping, error statuses, and the scratch guard on ragged sizes."""

import numpy as np
import pytest

import ancestral_reference as ar
import oracle
from comap_amd import engine, protein_models as pm, synthetic
from conftest import make_case
from tree_shapes import catalogue

pytestmark = pytest.mark.gpu

SHAPES = catalogue(2, 6)


def _eng(case, **kw):
    return engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"], **kw)


def _om(case):
    return oracle.Model(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])


def _check_oracle(r, o, min_clear=0.97):
    nodes = r["nodes"]
    post = o["post"][:, nodes].sum(axis=2).transpose(1, 0, 2)       # [n_inner, N, S]
    assert r["post"].shape == post.shape
    assert np.max(np.abs(r["post"] - post)) <= 1e-9
    clear = o["margin"][:, nodes].T > 1e-9
    assert clear.mean() >= min_clear, clear.mean()
    anc = o["anc"][:, nodes].T
    assert np.array_equal(r["states"][clear], anc[clear])


def _asr(eng, aln, masks=None):
    r = eng.ancestral_states(aln, masks=masks, want_posterior=True)
    s = eng.ancestral_states(aln, masks=masks)
    assert s["post"] is None and np.array_equal(s["states"], r["states"])
    assert r["states"].dtype == np.uint8
    return r


@pytest.mark.parametrize("S,ncat,seed", [(20, 4, 11), (4, 4, 12), (4, 2, 13)])
def test_make_case_with_unknowns_matches_oracle(S, ncat, seed):
    case = make_case(12, 300, S, seed, ncat=ncat)
    case["aln"][3, ::7] = S                                # unknowns at a leaf
    eng, om = _eng(case), _om(case)
    r = _asr(eng, case["aln"])
    assert r["nodes"] == ar.inner_nodes(case["parent"])
    _check_oracle(r, oracle.map_sites_marginal(om, case["aln"], True, want_post=True))


def test_myoglobin_matches_oracle(myo):
    Q, pi = pm.jtt92_bpp2x()
    rates, probs = pm.gamma_rates(float(myo["alpha"]), 4)
    eng = engine.Engine(myo["parent"], myo["blen"], myo["leaf_of_taxon"], Q, pi, rates, probs)
    r = _asr(eng, myo["aln"], masks=myo["masks"])
    assert len(r["nodes"]) == 98 and len(myo["masks"]) == 24
    om = oracle.Model(myo["parent"], myo["blen"], myo["leaf_of_taxon"], Q, pi, rates, probs)
    _check_oracle(r, oracle.map_sites_marginal(om, myo["aln"], True, masks=myo["masks"], want_post=True))


def _plain_case(S, seed=5):
    case = make_case(9, 70, 20, seed)
    Q, pi = pm.synthetic_reversible(S, seed + 100)
    rng = np.random.default_rng(seed)
    aln = rng.integers(0, S, size=case["aln"].shape).astype(np.uint8)
    base = rng.integers(0, S, size=(1, aln.shape[1]))
    aln = np.where(rng.random(aln.shape) < 0.6, base, aln).astype(np.uint8)
    aln[2, ::7] = S
    aln[5, 3::11] = 200
    case.update(Q=Q, pi=pi, aln=aln)
    return case


@pytest.mark.parametrize("S", [61, 64, 7])
def test_plain_alphabets_match_oracle(S):
    case = _plain_case(S)
    r = _asr(_eng(case), case["aln"])
    assert r["post"].shape[2] == S and r["states"].max() < S
    _check_oracle(r, oracle.map_sites_marginal(_om(case), case["aln"], True, want_post=True))


@pytest.mark.parametrize("model", ["protein_g4", "dna_g4"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_tree_shapes_match_oracle(shape, model):
    mdl = synthetic.protein_model(0.5, 4) if model == "protein_g4" else synthetic.dna_model(0.7, 4)
    S = len(mdl["pi"])
    blen = list(dict(shape.blen_variants()).values())[SHAPES.index(shape) % len(shape.blen_variants())]
    case = dict(parent=shape.parent, blen=blen, lot=shape.lot, **mdl)
    om = _om(case)
    sim, _ = oracle.simulate(om, 7 + shape.nn, 0, 40)
    rnd = np.random.default_rng(shape.nn).integers(0, S, size=(shape.ntaxa, 24)).astype(np.uint8)
    aln = np.ascontiguousarray(np.concatenate([sim, rnd], axis=1))
    r = _asr(_eng(case), aln)
    _check_oracle(r, oracle.map_sites_marginal(om, aln, True, want_post=True))


@pytest.mark.parametrize("S", [4, 20])
def test_model_set_matches_restatement(S):
    parent, blen, lot = synthetic.random_tree(10, 21 + S)
    Qs, pis, rf = ar.model_set(S, 3 + S)
    mob = (np.arange(len(parent)) % 2).astype(np.int32)
    rates, probs = pm.gamma_rates(0.6, 4)
    rng = np.random.default_rng(S)
    aln = rng.integers(0, S, size=(len(lot), 200)).astype(np.uint8)
    aln[:, :100] = aln[:1, :100]
    aln[4, ::9] = S
    eng = engine.Engine(parent, blen, lot, Qs, pis, rates, probs, model_of_branch=mob, root_freqs=rf)
    r = _asr(eng, aln)
    ref = ar.ancestral_states(parent, blen, lot, Qs, rates, probs, rf, aln, model_of_branch=mob)
    assert np.max(np.abs(r["post"] - ref["post"])) <= 1e-9
    top = np.sort(ref["post"], axis=2)
    clear = (top[:, :, -1] - top[:, :, -2]) > 1e-9 * top[:, :, -1]
    assert clear.mean() >= 0.97
    assert np.array_equal(r["states"][clear], ref["states"][clear])


# ------------------------------------------------------------------------------------------------ exact properties
@pytest.fixture(scope="module")
def target():
    """10 000 sites x 64 taxa, protein, JTT92 + Gamma4: the shape the pass budget is sized for (two passes)"""
    parent, blen, lot = synthetic.random_tree(64, 77)
    mdl = synthetic.protein_model(0.5, 4)
    case = dict(parent=parent, blen=blen, lot=lot, **mdl)
    aln, _ = oracle.simulate(_om(case), 78, 0, 10000)
    aln[7, ::13] = 20
    return case, np.ascontiguousarray(aln)


def _sites_per_pass(eng, case):
    per_site = 8 * 4 * len(case["rates"]) * len(case["parent"]) * (64 if eng.S not in (4, 20) else eng.S)
    return max(256, ((2 << 30) // per_site) // 256 * 256)


def test_target_crosses_a_pass_and_equals_ragged_sub_ranges(target):
    case, aln = target
    eng = _eng(case)
    assert _sites_per_pass(eng, case) < aln.shape[1] <= 2 * _sites_per_pass(eng, case)
    full = eng.ancestral_states(aln, want_posterior=True)
    cuts = [0, 1, 256, 257, 3333, 5121, 9999, 10000]
    parts = [eng.ancestral_states(aln[:, a:b], want_posterior=True) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(full["states"], np.concatenate([p["states"] for p in parts], axis=1))
    assert np.array_equal(full["post"], np.concatenate([p["post"] for p in parts], axis=1))
    idx = np.random.default_rng(1).choice(aln.shape[1], 500, replace=False)
    sub = np.ascontiguousarray(aln[:, idx])
    o = oracle.map_sites_marginal(_om(case), sub, True, want_post=True)
    _check_oracle(dict(nodes=full["nodes"], states=full["states"][:, idx], post=full["post"][:, idx]), o)


def test_side_stream_beside_the_null_equals_sequential():
    import torch
    case = make_case(20, 700, 20, 91)
    eng = _eng(case)
    dev = torch.device("cuda:0")
    d_aln = torch.from_numpy(case["aln"]).to(dev)
    nin, n = len(eng.inner_nodes()), case["aln"].shape[1]
    ram, nrep = 300, 3

    def run(overlap):
        states = torch.zeros(nin, n + 5, dtype=torch.uint8, device=dev)
        post = torch.zeros(nin, eng.S, n + 3, dtype=torch.float64, device=dev)
        stat = torch.zeros(nrep * ram, dtype=torch.float64, device=dev)
        nmin = torch.zeros(nrep * ram, dtype=torch.float64, device=dev)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        if overlap:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                eng.ancestral_states_dev(d_aln, states, post)
            eng.null_intra_dev(engine.STAT_CORRELATION, 9, 0, nrep, ram, stat, nmin=nmin)
            torch.cuda.current_stream().wait_stream(side)
        else:
            eng.ancestral_states_dev(d_aln, states, post)
            torch.cuda.synchronize()
            eng.null_intra_dev(engine.STAT_CORRELATION, 9, 0, nrep, ram, stat, nmin=nmin)
        torch.cuda.synchronize()
        return states.cpu().numpy(), post.cpu().numpy(), stat.cpu().numpy(), nmin.cpu().numpy()

    seq = run(False)
    host = eng.ancestral_states(case["aln"], want_posterior=True)
    assert np.array_equal(seq[0][:, :n], host["states"])
    assert np.array_equal(seq[1][:, :, :n], host["post"].transpose(0, 2, 1))
    for _ in range(2):
        for a, b in zip(seq, run(True)):
            assert np.array_equal(a, b, equal_nan=True)


def test_independent_of_mapping_options_and_weights_and_leaves_the_mapping_alone():
    case = make_case(14, 333, 20, 31)
    case["aln"][2, ::5] = 21
    masks = oracle.default_masks(20)[:23].copy()
    masks[21] = 0b1010
    eng = _eng(case)
    m0 = eng.map_sites(case["aln"], masks=masks)
    base = eng.ancestral_states(case["aln"], masks=masks, want_posterior=True)
    m1 = eng.map_sites(case["aln"], masks=masks)
    for k in m0:
        assert np.array_equal(m0[k], m1[k]), k
    eng.set_mapping_options(False, False)
    eng.set_statistic_weights(np.linspace(0.1, 2.0, eng.B))
    other = eng.ancestral_states(case["aln"], masks=masks, want_posterior=True)
    assert np.array_equal(base["states"], other["states"]) and np.array_equal(base["post"], other["post"])
    eng.set_mapping_options(True, True)
    eng.set_statistic_weights(None)
    plain = eng.map_sites(case["aln"])          # without the table: the leaf rows go back to "every state"
    ref = _eng(case).map_sites(case["aln"])
    for k in plain:
        assert np.array_equal(plain[k], ref[k]), k


def test_error_statuses():
    import torch
    case = make_case(8, 40, 20, 3)
    eng = _eng(case)
    lib, ctx = eng._lib, eng._ctx
    aln = np.ascontiguousarray(case["aln"])
    T, N = aln.shape
    nin = len(eng.inner_nodes())
    st = np.zeros((nin, N), dtype=np.uint8)
    vp, sz = engine._vp, engine._sz
    assert lib.cmx_ancestral_states(ctx, vp(aln), sz(N), sz(N), vp(None), sz(0), vp(None), vp(None)) == -1
    assert lib.cmx_ancestral_states(ctx, vp(aln), sz(0), sz(N), vp(None), sz(0), vp(st), vp(None)) == -1
    assert lib.cmx_ancestral_states(ctx, vp(aln), sz(N), sz(N - 1), vp(None), sz(0), vp(st), vp(None)) == -1
    bad = aln.copy()
    bad[0, 0] = 30
    masks = oracle.default_masks(20)[:23].copy()
    assert lib.cmx_ancestral_states(ctx, vp(bad), sz(N), sz(N), vp(masks), sz(23), vp(st), vp(None)) == -1
    assert lib.cmx_ancestral_states(ctx, vp(aln), sz(N), sz(N), vp(masks), sz(200), vp(st), vp(None)) == -2
    assert b"cmx_ancestral_states" in lib.cmx_last_error(ctx)
    dev = torch.device("cuda:0")
    d_aln = torch.from_numpy(aln).to(dev)
    d_st = torch.zeros(nin, N, dtype=torch.uint8, device=dev)
    d_post = torch.zeros(nin, 20, N, dtype=torch.float64, device=dev)
    strm = eng._stream()
    assert lib.cmx_ancestral_states_dev(ctx, vp(d_aln), sz(N), sz(N), vp(None), vp(None), sz(N), vp(None), sz(0), strm) == -1
    assert lib.cmx_ancestral_states_dev(ctx, vp(d_aln), sz(N), sz(N), vp(None), vp(d_st), sz(N - 1), vp(None), sz(0), strm) == -1
    assert lib.cmx_ancestral_states_dev(ctx, vp(d_aln), sz(N), sz(N), vp(None), vp(d_st), sz(N), vp(d_post), sz(N - 1), strm) == -1
    assert lib.cmx_ancestral_states_dev(ctx, vp(d_aln), sz(N), sz(N - 1), vp(None), vp(d_st), sz(N), vp(None), sz(0), strm) == -1
    pc = _plain_case(61)
    pe = _eng(pc)
    d_masks = torch.from_numpy(oracle.default_masks(20).astype(np.int32)).to(dev)
    d_pa = torch.from_numpy(np.ascontiguousarray(pc["aln"])).to(dev)
    d_ps = torch.zeros(len(pe.inner_nodes()), d_pa.shape[1], dtype=torch.uint8, device=dev)
    assert pe._lib.cmx_ancestral_states_dev(pe._ctx, vp(d_pa), sz(d_pa.shape[1]), sz(d_pa.shape[1]), vp(d_masks), vp(d_ps),
                                            sz(d_pa.shape[1]), vp(None), sz(0), pe._stream()) == -2
    pal = np.ascontiguousarray(pc["aln"])
    pst = np.zeros((len(pe.inner_nodes()), pal.shape[1]), dtype=np.uint8)
    assert pe._lib.cmx_ancestral_states(pe._ctx, vp(pal), sz(pal.shape[1]), sz(pal.shape[1]), vp(masks), sz(23), vp(pst),
                                        vp(None)) == -2
    torch.cuda.synchronize()
    # the failed calls did no device work: the context still gives what a fresh one gives
    assert np.array_equal(eng.ancestral_states(aln)["states"], _eng(case).ancestral_states(aln)["states"])


def test_ragged_sizes_under_the_scratch_guard(target):
    case, aln = target
    was = engine.scratch_guard(True)
    engine.scratch_guard_failures(clear=True)
    try:
        small = make_case(11, 300, 4, 41)
        es = _eng(small)
        for n in (1, 255, 257):
            r = es.ancestral_states(small["aln"][:, :n], want_posterior=True)
            assert r["states"].shape == (len(r["nodes"]), n)
        es.synchronize()
        es.scratch_check()
        eng = _eng(case)
        n = _sites_per_pass(eng, case) + 1
        big = np.ascontiguousarray(np.concatenate([aln, aln], axis=1)[:, :n])
        r = eng.ancestral_states(big, want_posterior=True)
        assert np.isfinite(r["post"]).all()
        eng.synchronize()
        eng.scratch_check()
        assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()
    finally:
        engine.scratch_guard(was)
