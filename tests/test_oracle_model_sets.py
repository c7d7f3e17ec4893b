"""The model-set oracle (oracle.ModelSet through oracle.c) proved on the CPU, before tests/test_gpu_model_sets.py holds the
device against it:

* collapse: a set of three copies of one generator with root_freqs = pi gives what the homogeneous Model gives;
* brute force: on the rooted 2-, 3- and 4-leaf shapes every mapping variant equals its definition, evaluated on the joint
  posterior from an enumeration of all state assignments (transition matrices from scipy's expm, counts from the numpy
  uniformization: nothing of oracle.c);
* distribution: simulated root states follow root_freqs, and a long branch follows its own generator;
* fragile share: of every simulator input of the GPU tests at most 1e-3 of the sites have a draw within 1e-9 of a boundary
  of its cumulative row (the sites those tests leave out);
* power: the restatement with model_of_branch forced to 0, or with the root drawn from pis[0], differs from itself in more
  than 1 % of the cells on every one of those inputs, and the mapping under generator 0 everywhere differs by more than
  1e-3 relative: a device that ignored the set could not pass."""
from functools import lru_cache

import numpy as np
import pytest
import scipy.linalg

import ancestral_reference as ar
import model_sets as ms
import oracle
from oracle import candidates as ocand, cluster as oc, np_oracle as npo
from comap_amd import synthetic
from conftest import rel_close
from tree_shapes import by_name, rooted_catalogue

FRAGILE_CAP = 1e-3


# ---------------------------------------------------------------------------------------------- collapse
@pytest.mark.parametrize("S", [4, 20])
def test_a_set_of_equal_generators_is_the_homogeneous_model(S):
    parent, blen, lot = ms.rooted_random_tree(7, 3)
    mdl = synthetic.dna_model(0.7, 3) if S == 4 else synthetic.protein_model(0.7, 3)
    rng = np.random.default_rng(S)
    hom = oracle.Model(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    hom2 = oracle.Model(parent, blen * 1.3, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])

    def as_set(b):
        return oracle.ModelSet(parent, b, lot, [mdl["Q"]] * 3, [mdl["pi"]] * 3, mdl["rates"], mdl["probs"],
                               rng.integers(0, 3, size=len(parent)), mdl["pi"])
    st, st2 = as_set(blen), as_set(blen * 1.3)
    a, c, near = oracle.simulate(st, 9, 7, 400, want_near=True)
    ah, ch = oracle.simulate(hom, 9, 7, 400)
    keep = ~ms.fragile(near)
    assert keep.mean() > 1 - FRAGILE_CAP
    assert np.array_equal(a[:, keep], ah[:, keep]) and np.array_equal(c[keep], ch[keep])
    a, r, near = oracle.simulate_continuous(st, 9, 7, 200, 0.8, 0.1, want_near=True)
    ah, rh = oracle.simulate_continuous(hom, 9, 7, 200, 0.8, 0.1)
    keep = ~ms.fragile(near)
    assert np.array_equal(r, rh) and np.array_equal(a[:, keep], ah[:, keep])
    aln = ah[:, :60].copy()
    aln[1, ::5] = S

    def same(x, y, exact=()):
        assert x.keys() == y.keys()
        for k in x:
            if x[k] is None:
                assert y[k] is None
            elif k in exact:
                assert np.array_equal(x[k], y[k]), k
            else:
                rel_close(x[k], y[k], 1e-10, 0.0)
    same(oracle.map_sites(st, aln), oracle.map_sites(hom, aln), ("rate_class",))
    same(oracle.map_sites_noavg(st, aln), oracle.map_sites_noavg(hom, aln), ("argmax",))
    for average in (True, False):
        same(oracle.map_sites_marginal(st, aln, average, want_post=True), oracle.map_sites_marginal(hom, aln, average, want_post=True),
             ("anc",))
    same(oracle.null_intra(st, 0, 5, 1, 3, 20), oracle.null_intra(hom, 0, 5, 1, 3, 20), ("rcmin",))
    sup = np.stack([np.stack([ah[:, 100 + 20 * (2 * r + h):120 + 20 * (2 * r + h)] for h in range(2)]) for r in range(2)])
    same(oracle.null_intra(st, 1, 0, 0, 2, 20, supplied=sup), oracle.null_intra(hom, 1, 0, 0, 2, 20, supplied=sup), ("rcmin",))
    same(oracle.null_inter(st, st2, 0, 5, 0, 2, 20), oracle.null_inter(hom, hom2, 0, 5, 0, 2, 20), ("rcmin",))


# ---------------------------------------------------------------------------------------------- brute force
def _conditional_counts(Q, Bm, t):
    """N(x, y; t) = J / P with P from expm and J from the numpy uniformization"""
    return npo.conditional_counts(npo.count_matrix_uniformization(Q, Bm, t), scipy.linalg.expm(Q * t), True)


@pytest.mark.parametrize("shape", ms.SHAPES)
def test_the_mappings_of_a_set_equal_their_definitions_by_enumeration(shape):
    sh = by_name(shape, rooted_catalogue(2, 4))
    c = ms.case("n4x2:" + shape)
    S, C, nn = 4, 2, sh.nn
    assert len(c["rates"]) == C and c["mob"][np.flatnonzero(c["parent"] == nn - 1)[:2]].tolist() == [0, 1]
    assert all(np.abs(c["root"] - p).max() > 0.01 for p in c["pis"])
    om = ms.oracle_of(c)
    rng = np.random.default_rng(nn)
    aln = rng.integers(0, S, size=(sh.ntaxa, 14)).astype(np.uint8)
    aln[:, :4] = aln[0, :4]                                # some constant columns
    aln[0, 5], aln[-1, 6] = 4, 11                          # R (A or G) and D (A, G or T)
    bf = ar.brute_force_joint(c["parent"], c["blen"], c["lot"], c["Qs"], c["rates"], c["probs"], c["root"], aln, ms.IUPAC,
                              c["mob"])
    L = bf["L"]
    pair, node = bf["pair"] / L[None, None, :, None, None], bf["node"] / L[None, None, :, None]
    leaf = np.zeros(nn, dtype=bool)
    leaf[c["lot"]] = True
    for b in np.flatnonzero(leaf):                         # the leaf rule of the marginal variants: e(x) p_c / sum(e)
        e = (node[b].sum(0) > 0).astype(float)
        node[b] = c["probs"][:, None, None] * (e / e.sum(1, keepdims=True))[None]
    Bm = ms.registers(c)[:, 0]
    N = aln.shape[1]
    avg, mavg, noavg, mnoavg = (np.zeros((N, nn - 1)) for _ in range(4))
    for b in range(nn - 1):
        g, f = c["mob"][b], c["parent"][b]
        N1 = _conditional_counts(c["Qs"][g], Bm[g], c["blen"][b])
        for k, r in enumerate(c["rates"]):
            Nc = _conditional_counts(c["Qs"][g], Bm[g], c["blen"][b] * r)
            avg[:, b] += np.einsum("ixy,xy->i", pair[b, k], Nc)
            mavg[:, b] += np.einsum("ix,xy,iy->i", node[f, k], Nc, node[b, k])
        pxy = pair[b].sum(0).reshape(N, S * S)
        noavg[:, b] = N1.ravel()[np.argmax(pxy, axis=1)]
        xf, xb = np.argmax(node[f].sum(0), axis=1), np.argmax(node[b].sum(0), axis=1)
        mnoavg[:, b] = N1[xf, xb]
    o = oracle.map_sites(om, aln, ms.IUPAC)
    rel_close(o["logL"], np.log(L), 1e-10)
    rel_close(o["counts"][:, :, 0], avg, 1e-10, 1e-14)
    post = bf["node"][-1].sum(-1) / L[None]                # Pr(class | data)
    assert np.array_equal(o["rate_class"], np.argmax(post, axis=0))
    rel_close(o["post_rate"], (c["rates"][:, None] * post).sum(0), 1e-10)
    rel_close(oracle.map_sites_marginal(om, aln, True, ms.IUPAC)["counts"][:, :, 0], mavg, 1e-10, 1e-14)
    on = oracle.map_sites_noavg(om, aln, ms.IUPAC)
    clear = on["margin"] > 1e-9
    rel_close(on["counts"][:, :, 0][clear], noavg[clear], 1e-10, 1e-14)
    om_ = oracle.map_sites_marginal(om, aln, False, ms.IUPAC)
    clear = (om_["margin"][:, :-1] > 1e-9) & (om_["margin"][:, c["parent"][:-1]] > 1e-9)
    assert clear.mean() > 0.8
    rel_close(om_["counts"][:, :, 0][clear], mnoavg[clear], 1e-10, 1e-14)


# ---------------------------------------------------------------------------------------------- distribution
def test_simulated_states_follow_the_root_frequencies_and_the_branch_generator():
    c = dict(ms.case("n4x4:(x,x)"))
    n, S = 40000, 4
    leaf_a, leaf_b = int(c["lot"][0]), int(c["lot"][1])
    # near-zero branches: both leaves show the root state
    c["blen"] = np.array([1e-9, 1e-9, 0.0])
    a, _ = oracle.simulate(ms.oracle_of(c), 11, 0, n)
    freq = np.bincount(a[0], minlength=S) / n
    se = np.sqrt(c["root"] * (1 - c["root"]) / n)
    assert np.all(np.abs(freq - c["root"]) < 4 * se), (freq, c["root"])
    assert np.any(np.abs(freq - c["pis"][0]) > 4 * se)     # and not the frequencies of generator 0
    # one long leaf branch on a generator other than 0: its table given the father's state (shown by the other leaf)
    blen = np.zeros(3)
    blen[leaf_a], blen[leaf_b] = 1e-9, 0.8
    c["blen"] = blen
    mob = c["mob"].copy()
    mob[leaf_b] = 2
    c["mob"] = mob
    a, _ = oracle.simulate(ms.oracle_of(c), 12, 0, n)
    x, y = a[0], a[1]
    table = np.zeros((S, S))
    np.add.at(table, (x, y), 1)

    def expected(g):
        return sum(p * scipy.linalg.expm(c["Qs"][g] * 0.8 * r) for r, p in zip(c["rates"], c["probs"]))
    rows = table.sum(1, keepdims=True)
    big = expected(2) * rows >= 50
    assert big.sum() >= 12
    se = np.sqrt(expected(2) * (1 - expected(2)) / rows)
    assert np.all(np.abs(table / rows - expected(2))[big] < 4 * se[big])
    assert np.any(np.abs(table / rows - expected(0))[big] > 4 * se[big])


# ---------------------------------------------------------------------------------------------- fragile share and power
def _mutants(c):
    """the two ways of ignoring the set: generator 0 on every branch; the root drawn from the frequencies of generator 0"""
    return [ms.oracle_of(c, mob=np.zeros_like(c["mob"])), ms.oracle_of(c, root=c["pis"][0])]


@lru_cache(maxsize=None)
def _figures():
    """label -> (fragile share, smallest share of cells that a mutant simulator changes) over every simulator input"""
    out = {}
    for label, c, seed, g0, n in ms.discrete_inputs():
        a, cl, near = oracle.simulate(ms.oracle_of(c), seed, g0, n, want_near=True)
        out[label] = (ms.fragile(near).mean(), min((oracle.simulate(m, seed, g0, n)[0] != a).mean() for m in _mutants(c)))
    for label, c, seed, g0, n, alpha, pinv in ms.continuous_inputs():
        a, r, near = oracle.simulate_continuous(ms.oracle_of(c), seed, g0, n, alpha, pinv, want_near=True)
        out[label] = (ms.fragile(near).mean(),
                      min((oracle.simulate_continuous(m, seed, g0, n, alpha, pinv)[0] != a).mean() for m in _mutants(c)))
    return out


def test_fragile_sites_are_rare_in_every_simulator_input_of_the_gpu_tests():
    fig = _figures()
    worst = max(fig, key=lambda k: fig[k][0])
    print("largest fragile share: %.3g (%s)" % (fig[worst][0], worst))
    assert all(f <= FRAGILE_CAP for f, _ in fig.values()), {k: v[0] for k, v in fig.items() if v[0] > FRAGILE_CAP}


def test_a_simulator_that_ignored_the_set_changes_more_than_a_hundredth_of_the_cells():
    fig = _figures()
    weakest = min(fig, key=lambda k: fig[k][1])
    print("smallest simulator power: %.3g of the cells (%s)" % (fig[weakest][1], weakest))
    assert all(p > 0.01 for _, p in fig.values()), {k: v[1] for k, v in fig.items() if v[1] <= 0.01}


@pytest.mark.parametrize("name", ms.MAPPING_CASES)
def test_a_mapping_under_generator_zero_differs(name):
    c = ms.case(name)
    aln = ms.alignment(c)
    o = oracle.map_sites(ms.oracle_of(c), aln)["counts"]
    z = oracle.map_sites(ms.oracle_of(c, mob=np.zeros_like(c["mob"])), aln)["counts"]
    rel = np.abs(z - o).max() / np.abs(o).max()
    print("mapping power %s: %.3g" % (name, rel))
    assert rel > 1e-3


# ---------------------------------------------------------------------------------------------- composed oracles
def test_the_composed_oracles_take_a_set():
    c = ms.case("n4x4")
    om = ms.oracle_of(c)
    o = oc.cluster_null(om, oc.DIST_CORRELATION, oc.LINK_COMPLETE, 3, 0, 1, 20)
    a, _ = oracle.simulate(om, 3, 0, 20)
    counts = oracle.map_sites(om, a)["counts"]
    merge, dmax, _ = oc.hclust(oc.distance_matrix(oc.DIST_CORRELATION, counts), oc.LINK_COMPLETE)
    assert np.array_equal(o[0]["merge"], merge) and np.array_equal(o[0]["dmax"], dmax)
    norm = oracle.map_sites(om, a)["norm"]
    win = [[(norm[i] - 0.5, norm[i] + 0.5) for i in g] for g in ([0, 1], [2, 3, 4])]
    r = ocand.candidate_groups(om, 0, win, [1, 1], [0.1, 0.1], min_sim=5, rep_ram=32, max_trials=3, seed=1)
    assert np.all(r["n2"] <= 5) and r["batches"] >= 1
