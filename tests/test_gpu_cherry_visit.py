"""-m gpu: the outside visit of an inlined cherry that keeps its leaf rows in registers (cmx_walk.h, kCherryRows) against
the oracle, on the smallest trees that hold every case of it:

    ((x,x),x)        the cherry is child A beside a leaf        (x,(x,x))      child B beside a leaf
    ((x,x),(x,x))    two cherries under one parent              (((x,x),x),x)  the cherry beside a visited, handed sibling
    unrooted7        random_tree's 7 taxa with a trifurcating root (pseudo nodes)

70 sites: one full wave of 64 and a partial one.  Every unfused instantiation of the mapping kernel takes the visit:
* protein, 4 rate classes: at this size the observed mapping is the 16-site class-split launch; the null runs the fused
  kernel over sites and over patterns, which must give the same bytes;
* protein, one rate class: the observed mapping in 64-site waves;
* DNA, 3 rate classes (not class-fused) and two substitution types: the K loops of the visit, class-split observed
  launch, null over sites and over patterns.
The observed alignments carry ambiguity codes (a two-state code and the unknown) in the leaves of every cherry, also in
both leaves of a cherry at once.  Tolerances are those of tests/test_gpu_tiny_trees.py for the same quantities."""
import numpy as np
import pytest

import oracle
from comap_amd import engine, synthetic
from conftest import rel_close
from test_gpu_parity import _check_map
from test_gpu_tiny_trees import _null_degenerate, _null_vectors, _stat_close
from tree_shapes import by_name, catalogue

pytestmark = pytest.mark.gpu

_CATALOGUE = catalogue(2, 7)
NAMES = ["((x,x),x)", "(x,(x,x))", "((x,x),(x,x))", "(((x,x),x),x)", "unrooted7"]
MODELS = ["protein_g4", "protein_1cls", "dna_3cls_2types"]
KEYS = ("stat", "rcmin", "prmin", "nmin")
NSITES = 70


def _model(name):
    """-> (model dict, Bk or None)"""
    if name == "protein_g4":
        return synthetic.protein_model(0.5, 4), None
    if name == "protein_1cls":
        return synthetic.protein_model(0.5, 1), None
    m = synthetic.dna_model(0.7, 3)
    W1 = np.random.default_rng(4).uniform(-1, 1, size=(4, 4))
    return m, np.stack([synthetic.weighted_register(m["Q"], W1), synthetic.weighted_register(m["Q"], np.abs(W1))])


def _cherry_taxa(shape):
    """taxa of the leaves of the inlined cherries, one pair per cherry"""
    kids, taxon = shape.children(), {int(n): t for t, n in enumerate(shape.lot)}
    return [(taxon[kids[c][0]], taxon[kids[c][1]]) for c in shape.cherries()]


def _alignment(om, shape, S, seed):
    """46 simulated columns + 24 uniform random ones; ambiguity codes S (two states) and S + 1 (unknown) in the cherries'
    leaves: each leaf alone and both leaves of a cherry together.  -> (alignment, mask table)"""
    sim, _ = oracle.simulate(om, seed, 0, NSITES - 24)
    rng = np.random.default_rng(seed)
    aln = np.ascontiguousarray(np.concatenate([sim, rng.integers(0, S, size=(shape.ntaxa, 24)).astype(np.uint8)], axis=1))
    masks = oracle.default_masks(S)
    masks[S] = (1 << 1) | (1 << (S - 1))
    pairs = _cherry_taxa(shape)
    assert pairs
    for i, (t1, t2) in enumerate(pairs):
        cols = rng.permutation(NSITES)
        aln[t1, cols[:8]] = S
        aln[t2, cols[8:16]] = S + 1
        aln[t1, cols[16:22]] = S + 1            # both leaves of the cherry ambiguous
        aln[t2, cols[16:22]] = S
    aln[pairs[0][0], 63:66] = S                   # across the edge of the first wave
    return aln, masks


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", NAMES)
def test_cherry_visit_against_the_oracle(name, model):
    shape = by_name(name, _CATALOGUE)
    mdl, Bk = _model(model)
    S = len(mdl["pi"])
    idx = NAMES.index(name) + MODELS.index(model)
    vs = shape.blen_variants()
    blen = vs[idx % len(vs)][1]                   # the branch-length variants rotate over shapes and models
    kw = {} if Bk is None else dict(Bk=Bk)
    eng = engine.Engine(shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"],
                        clamp_negative=Bk is None, **kw)
    om = oracle.Model(shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"], nonneg=Bk is None, **kw)
    assert eng.info()["cherry_tables"] == 0       # unfused: no table walk, the row-reusing visit
    # ---- observed mapping, ambiguity codes in the cherries' leaves
    aln, masks = _alignment(om, shape, S, 300 + idx)
    _check_map(eng.map_sites(aln, masks=masks[: S + 2]), oracle.map_sites(om, aln, masks))
    # ---- the fused null over sites and over patterns: the same bytes, and the oracle's values
    kind = engine.STAT_CORRELATION if Bk is None else engine.STAT_COMPENSATION
    nrep, ram, seed = 2, NSITES, 11 + idx
    eng.set_null_patterns(False)
    off = eng.null_intra(kind, seed, 0, nrep, ram)
    eng.set_null_patterns(True)
    on = eng.null_intra(kind, seed, 0, nrep, ram)
    eng.set_null_patterns(None)
    for k in KEYS:
        assert off[k].tobytes() == on[k].tobytes(), k
    o = oracle.null_intra(om, kind, seed, 0, nrep, ram)
    deg = _null_degenerate(_null_vectors(om, seed, nrep, ram)) if kind == engine.STAT_CORRELATION else np.zeros(nrep * ram, bool)
    _stat_close(off["stat"], o["stat"], deg)
    rel_close(off["nmin"], o["nmin"], 1e-6)
    rel_close(off["prmin"], o["prmin"], 1e-9)
    assert np.array_equal(off["rcmin"], o["rcmin"])
    eng.synchronize()
