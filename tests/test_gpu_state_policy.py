"""-m gpu: every global access of per-wave state in the mapping kernel (cmx_map.hip: state_load / state_store /
store_vec / load_vec with a compile-time cache policy) once, on the smallest inputs that reach it.

A cache-policy bit does not touch a value, so the checks are the plain ones: the oracle at test_gpu_parity's tolerances,
and every call made twice with equal bytes.

NONE OF THESE TESTS CAN PROVE THE COHERENCE RULE (a location stored with a form that bypasses the CU's L1 is loaded only
with a form that bypasses it too).  A violation shows only when a plain load hits the line an earlier class pass left in
the L1, and the walk's other traffic evicts that line almost always: a wrong build passes here.  The rule holds by
construction -- StatePolicy's static_asserts and the reader table of DESIGN 4.1 -- and these tests only show that the
helpers move the right bytes on every path.

Trees: `root6` of lds_slot_trees.py, ((a,(b,c)),(d,(e,f))), the smallest tree with a node whose two children are both
visited: a pass has workspace stores and loads (V) and the LDS slot is planned (asserted below).  No six-taxon UNROOTED
tree has such a node (tree_shapes' `unrooted6` plans nothing: its trifurcating root leaves one visited child per
node); it runs too, for the walk without the slot.

* every class once: protein Gamma-4, 70 sites = one full 64-site block and a partial one.  Paths: the class-split
  launch (S: 70 sites are 16-site wave-tasks), the all-class observed kernel (V, P, T: the 70 columns repeated past the
  512 wave-tasks up to which the split launch is taken, ending in a partial block), the fused null per site and per
  distinct pattern (V, P, T).
* all instantiations: the same for class-fused DNA Gamma-4 (16 device states, one device class: every observed
  alignment takes the all-class kernel) and a 4-state Gamma-3 model.
* slot reuse across blocks: info()["waves"] x 64 + 64 sites made of one 64-column block repeated, so that every wave of
  the observed grid maps several blocks through the same workspace slots; every block equals block 0 byte for byte and
  block 0 agrees with the oracle."""
import functools

import numpy as np
import pytest

import oracle
from comap_amd import engine, synthetic
from conftest import rel_close
from lds_slot_trees import hand_built
from test_gpu_parity import _check_map
from tree_shapes import by_name

pytestmark = pytest.mark.gpu

NSITES, NREP, RAM = 70, 3, 70
MODELS = {"protein_g4": lambda: synthetic.protein_model(0.5, 4), "dna_g4_fused": lambda: synthetic.dna_model(0.5, 4),
          "dna_g3": lambda: synthetic.dna_model(0.5, 3)}
NULL_KEYS = ("stat", "nmin", "prmin", "rcmin")


@functools.lru_cache(maxsize=None)
def _shape(name):
    return [s for s in hand_built() if s.name == name][0] if name == "root6" else by_name(name)


@functools.lru_cache(maxsize=None)
def _case(tree, model):
    """-> (engine arguments, oracle model, 70 simulated columns, the oracle's mapping of them, the oracle's null): made
    once per (tree, model) and left unchanged"""
    shape, mdl = _shape(tree), MODELS[model]()
    blen = np.random.default_rng(shape.nn).uniform(0.05, 0.4, size=shape.nn)
    blen[-1] = 0.0
    args = (shape.parent, blen, shape.lot, mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    om = oracle.Model(*args)
    cols, _ = oracle.simulate(om, 17, 0, NSITES)
    cols = np.ascontiguousarray(cols)
    return args, om, cols, oracle.map_sites(om, cols), oracle.null_intra(om, oracle.ST_CORRELATION, 7, 0, NREP, RAM)


def _twice(call, what):
    a, b = call(), call()
    for key in a:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (what, key)
    return a


def _check_null(got, want):
    rel_close(got["stat"], want["stat"], 1e-6, 1e-12)
    rel_close(got["nmin"], want["nmin"], 1e-6)
    rel_close(got["prmin"], want["prmin"], 1e-9)
    assert np.array_equal(got["rcmin"], want["rcmin"])


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("tree", ["root6", "unrooted6"])
def test_every_path_against_the_oracle_and_itself(tree, model):
    args, om, cols, want_map, want_null = _case(tree, model)
    if tree == "root6" and model == "protein_g4":
        walk = engine.debug_walk(*args)
        assert walk["stores"] > 0 and walk["loads"] > 0 and walk["lds_loads"] > 0 and walk["lds_stores"] > 0
    eng = engine.Engine(*args)
    info = eng.info()
    # ---- 70 sites: the class-split launch wherever the device model has more than one class
    _check_map(_twice(lambda: eng.map_sites(cols), "70 sites"), want_map)
    # ---- the all-class observed kernel: more (64-site block, class) tasks than the observed grid has waves (a quarter
    # of the resident waves), the last block partial
    if info["device_classes"] > 1:
        n = ((info["waves"] // 4) // info["device_classes"] + 1) * 64 + 6
        rep = np.arange(n) % NSITES
        got = _twice(lambda: eng.map_sites(np.ascontiguousarray(cols[:, rep])), "all-class observed")
        _check_map(got, {k: v[rep] for k, v in want_map.items()})
    # ---- the fused null, per site and per distinct pattern
    for patterns in (False, True):
        eng.set_null_patterns(patterns)
        got = _twice(lambda: eng.null_intra(engine.STAT_CORRELATION, 7, 0, NREP, RAM), "null, patterns %s" % patterns)
        _check_null({k: got[k] for k in NULL_KEYS}, want_null)
    eng.synchronize()
    eng.close()


def test_slot_reuse_across_blocks():
    """one 64-column block repeated over more blocks than there are waves: a wave maps its blocks one after another
    through the same workspace slots, `part` and count block; each must come out as the first did"""
    args, om, cols, want_map, _ = _case("root6", "protein_g4")
    eng = engine.Engine(*args)
    block = cols[:, :64]
    nblocks = eng.info()["waves"] + 1
    got = _twice(lambda: eng.map_sites(np.ascontiguousarray(np.tile(block, (1, nblocks)))), "repeated block")
    for key, v in got.items():
        v = np.asarray(v)
        blocks = v.reshape((nblocks, 64) + v.shape[1:])      # (the site is the first axis of every output)
        assert np.ascontiguousarray(np.broadcast_to(blocks[:1], blocks.shape)).tobytes() == blocks.tobytes(), key
    _check_map({k: np.asarray(v)[:64] for k, v in got.items()}, {k: v[:64] for k, v in want_map.items()})
    eng.synchronize()
    eng.close()
