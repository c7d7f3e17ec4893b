"""The trees beyond fp64's range that tests/test_scaled_reference.py (CPU) and tests/test_gpu_likelihood_scaling.py share,
a plain helper module.  Every case is built once per process, with the fp64 operators of tests/scaled_reference.py and a
cache of that reference's results.

    long(S, T)    synthetic.random_tree(T, 77) with branch lengths x 25, 8 sites of oracle.simulate(om, 78, 0, 8);
                  (S, T) in LONG: 3, 4 and 4 of the 8 sites have logL = -inf in the C oracle, (20, 600) needs more than one
                  rescale per site
    star()        a root with 320 leaf children, protein, branch length 2.0: a single node's product underflows
    multi()       test_traversal_program._random_multifurcating(300, 5), protein, branch lengths x 25
"""
from functools import lru_cache

import numpy as np

import oracle
import scaled_reference as sr
from comap_amd import synthetic

LONG = [(20, 300), (4, 600), (20, 600)]
OPTIONS = [(True, True), (False, True), (True, False), (False, False)]      # (nijt.average, nijt.joint)


class Case:
    def __init__(self, name, parent, blen, lot, S, nsites=8, seed=78):
        mdl = synthetic.protein_model(0.5, 4) if S == 20 else synthetic.dna_model(0.5, 4)
        self.name, self.parent, self.blen, self.lot, self.S = name, parent, blen, lot, S
        self.Q, self.pi, self.rates, self.probs = mdl["Q"], mdl["pi"], np.asarray(mdl["rates"]), np.asarray(mdl["probs"])
        self.om = oracle.Model(parent, blen, lot, self.Q, self.pi, self.rates, self.probs)
        self.aln = np.ascontiguousarray(oracle.simulate(self.om, seed, 0, nsites)[0])
        self._ops, self._ref = None, {}

    def model_args(self):
        return (self.parent, self.blen, self.lot, self.Q, self.pi, self.rates, self.probs)

    def ops(self):
        if self._ops is None:
            self._ops = sr.operators(self.parent, self.blen, self.Q, self.pi, self.rates)
        return self._ops

    def _args(self, aln):
        return (self.parent, self.blen, self.lot, self.aln if aln is None else aln, self.Q, self.pi, self.rates, self.probs)

    def reference(self, average=True, joint=True, dtype=np.float64, scale=True):
        """scaled_reference.map_sites of the case's own alignment (cached; do not write to it)"""
        key = (average, joint, np.dtype(dtype).name, scale)
        if key not in self._ref:
            self._ref[key] = sr.map_sites(*self._args(None), ops=self.ops(), average=average, joint=joint, dtype=dtype, scale=scale)
        return self._ref[key]

    def map(self, aln, **kw):
        return sr.map_sites(*self._args(aln), ops=self.ops(), **kw)

    def ancestral(self, dtype=np.float64, scale=True):
        key = ("asr", np.dtype(dtype).name, scale)
        if key not in self._ref:
            self._ref[key] = sr.ancestral_states(*self._args(None), ops=self.ops(), dtype=dtype, scale=scale)
        return self._ref[key]

    def engine(self, **kw):
        from comap_amd import engine
        return engine.Engine(*self.model_args(), **kw)


@lru_cache(maxsize=None)
def long(S, T):
    parent, blen, lot = synthetic.random_tree(T, 77)
    return Case(f"long{S}x{T}", parent, blen * 25.0, lot, S)


@lru_cache(maxsize=None)
def star(nleaves=320, blen=2.0):
    parent = np.full(nleaves + 1, nleaves, dtype=np.int32)
    parent[-1] = -1
    bl = np.full(nleaves + 1, blen)
    bl[-1] = 0.0
    return Case("star", parent, bl, np.arange(nleaves, dtype=np.int32), 20)


@lru_cache(maxsize=None)
def multi():
    from test_traversal_program import _random_multifurcating
    parent, blen, lot = _random_multifurcating(300, 5)
    return Case("multi", parent, blen * 25.0, lot, 20)
