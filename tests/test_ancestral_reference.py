"""asr.method = marginal (CoMap/CoMap.cpp:169-197) without a GPU: the numpy restatement (tests/ancestral_reference.py) is
pinned to the definition by brute force over every internal assignment, and to the oracle's marginal states and
posteriors (oracle.map_sites_marginal, itself pinned by tests/test_oracle_marginal.py); the library exports the entry
points; the Fasta writer of output.sequence.file prints the text it should."""
import numpy as np
import pytest

import ancestral_reference as ar
import oracle
from comap_amd import engine, formats, protein_models, synthetic
from tree_shapes import catalogue

SMALL = [s for s in catalogue(2, 5)]


def _alignment(S, T, N, seed, unknown=False):
    rng = np.random.default_rng(seed)
    aln = rng.integers(0, S, size=(T, N)).astype(np.uint8)
    aln[:, :3] = aln[:1, :3]               # a few conserved columns
    if unknown:
        aln[0, 1::4] = S                   # an unknown at a leaf
    return aln


@pytest.mark.parametrize("shape", SMALL, ids=[s.name for s in SMALL])
def test_restatement_equals_brute_force_dna(shape):
    mdl = synthetic.dna_model(0.7, 3)
    blen = np.where(np.asarray(shape.parent) >= 0, 0.05 + 0.3 * np.random.default_rng(shape.nn).random(shape.nn), 0.0)
    aln = _alignment(4, shape.ntaxa, 9, shape.nn, unknown=True)
    r = ar.ancestral_states(shape.parent, blen, shape.lot, mdl["Q"], mdl["rates"], mdl["probs"], mdl["pi"], aln)
    bf = ar.brute_force(shape.parent, blen, shape.lot, mdl["Q"], mdl["rates"], mdl["probs"], mdl["pi"], aln)
    assert r["nodes"] == [n for n in range(shape.nn) if n not in set(int(x) for x in shape.lot)]
    assert np.allclose(r["post"], bf, rtol=0, atol=1e-12)
    assert np.allclose(r["post"].sum(axis=2), 1.0, atol=1e-12)


@pytest.mark.parametrize("shape", [s for s in SMALL if s.nn - s.ntaxa <= 2], ids=lambda s: s.name)
def test_restatement_equals_brute_force_protein(shape):
    mdl = synthetic.protein_model(0.5, 4)
    blen = np.where(np.asarray(shape.parent) >= 0, 0.2, 0.0)
    aln = _alignment(20, shape.ntaxa, 5, 3 + shape.nn)
    r = ar.ancestral_states(shape.parent, blen, shape.lot, mdl["Q"], mdl["rates"], mdl["probs"], mdl["pi"], aln)
    bf = ar.brute_force(shape.parent, blen, shape.lot, mdl["Q"], mdl["rates"], mdl["probs"], mdl["pi"], aln)
    assert np.allclose(r["post"], bf, rtol=0, atol=1e-12)


@pytest.mark.parametrize("shape", [s for s in SMALL if s.ntaxa >= 3][:8], ids=lambda s: s.name)
def test_restatement_equals_brute_force_model_set(shape):
    Qs, _, rf = ar.model_set(4, shape.nn)
    mob = np.arange(shape.nn) % 2
    rates, probs = protein_models.gamma_rates(0.6, 3)
    blen = np.where(np.asarray(shape.parent) >= 0, 0.15, 0.0)
    aln = _alignment(4, shape.ntaxa, 7, shape.nn + 1)
    r = ar.ancestral_states(shape.parent, blen, shape.lot, Qs, rates, probs, rf, aln, model_of_branch=mob)
    bf = ar.brute_force(shape.parent, blen, shape.lot, Qs, rates, probs, rf, aln, model_of_branch=mob)
    assert np.allclose(r["post"], bf, rtol=0, atol=1e-12)


@pytest.mark.parametrize("S,ncat,seed", [(4, 4, 3), (20, 4, 5), (4, 2, 8)])
def test_restatement_equals_the_oracle(S, ncat, seed):
    parent, blen, lot = synthetic.random_tree(9, seed)
    mdl = synthetic.protein_model(0.5, ncat) if S == 20 else synthetic.dna_model(0.7, ncat)
    om = oracle.Model(parent, blen, lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    aln, _ = oracle.simulate(om, seed, 0, 60)
    aln[2, ::5] = S                        # unknowns at a leaf
    o = oracle.map_sites_marginal(om, aln, True, want_post=True)
    r = ar.ancestral_states(parent, blen, lot, mdl["Q"], mdl["rates"], mdl["probs"], mdl["pi"], aln)
    nodes = r["nodes"]
    opost = o["post"][:, nodes].sum(axis=2).transpose(1, 0, 2)      # [n_inner, N, S]
    assert np.allclose(r["post"], opost, rtol=0, atol=1e-12)
    clear = o["margin"][:, nodes].T > 1e-9
    assert np.array_equal(r["states"][clear], o["anc"][:, nodes].T[clear])


def test_library_and_engine_expose_the_ancestral_states():
    lib = engine.load_library()
    for name in ("cmx_ancestral_states", "cmx_ancestral_states_dev"):
        assert hasattr(lib, name) and name in engine.EXPORTS
    assert callable(getattr(engine.Engine, "ancestral_states", None))
    assert callable(getattr(engine.Engine, "ancestral_states_dev", None))


def test_fasta_writer_text():
    states = np.array([[0, 1, 2, 3, 4], [3, 3, 2, 1, 0]], dtype=np.uint8)
    aln = np.array([[0, 0, 9, 1, 2], [1, 2, 3, 0, 255]], dtype=np.uint8)
    text = formats.to_text(formats.write_ancestral_fasta, [5, 7], states, ["seqA", "seqB"], aln, nstates=4)
    assert text == ">5\nACGTN\n>7\nTTGCA\n>seqA\nAANCG\n>seqB\nCGTAN\n"


def test_fasta_writer_wraps_at_100_and_names_nodes():
    N = 250
    states = (np.arange(N) % 21).astype(np.uint8)[None]
    aln = np.zeros((1, N), dtype=np.uint8)
    text = formats.to_text(formats.write_ancestral_fasta, [12], states, ["leaf"], aln, nstates=20, node_names=["n12"])
    seq = "".join((protein_models.AA_ORDER + "X")[i % 21] for i in range(N))
    assert text == ">n12\n" + seq[:100] + "\n" + seq[100:200] + "\n" + seq[200:] + "\n>leaf\n" + "A" * 100 + "\n" + \
        "A" * 100 + "\n" + "A" * 50 + "\n"
    assert formats.to_text(formats.write_ancestral_fasta, [0], states[:, :3], [], aln[:0], symbols=["AAA", "AAC", "AAG"],
                           unknown="NNN") == ">0\nAAAAACAAG\n"
    with pytest.raises(ValueError):
        formats.to_text(formats.write_ancestral_fasta, [0], states, [], aln[:0], nstates=61)
