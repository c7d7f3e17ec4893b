"""-m gpu: the default mapping under likelihood scaling on the f64 matrix instruction (cmx_map_wide.hip at 64 device states,
cmx_map_wide20.hip at 20).

With cmx_set_likelihood_scaling the default mapping (nijt.average = yes, nijt.joint = yes) and its site scalars run
matrix-core kernels at 20 states and at every alphabet other than 4 states; cmx_debug_map_scaled_plain(1) forces the scaled
plain kernels.  Here: both paths against tests/scaled_reference.py (uint32 masks: up to 32 states, so 21 states stand for the
64-state shape) or, at 61 states under underflow, against each other; nothing underflows: the oracle and the unscaled call;
tiles; tree shapes; model sets; the kernels this leaves alone, as bytes; the null and the two-stream use; the scratch guard.

Tolerances: the project's plain-kernel bars throughout (_check_plain of tests/test_gpu_likelihood_scaling.py): counts and
norm 1e-9 (atol 1e-300), logL and post_rate 1e-12, rate_class equal.  Every input that is meant to underflow asserts that
the unscaled computation loses sites on it (the C oracle's; at 61 states the engine's own unscaled mapping)."""
from functools import lru_cache

import numpy as np
import pytest

import model_sets as ms
import oracle
import scaled_cases as sc
import scaled_reference as sr
from comap_amd import engine, protein_models as pm, synthetic
from conftest import make_case, rel_close
from test_gpu_codon_alphabets import _case
from test_gpu_likelihood_scaling import _check_plain, _masked_protein_case
from test_gpu_map_wide import _shape, _two_types

pytestmark = pytest.mark.gpu

KEYS = ("counts", "norm", "logL", "post_rate", "rate_class")


class scaled_plain:
    """with scaled_plain(on): the switch set for the block, the previous state back afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = engine.map_scaled_plain(self.on)

    def __exit__(self, *exc):
        engine.map_scaled_plain(self.was)


def _same_bytes(a, b, what="", keys=KEYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _finite(r, what=""):
    for k in KEYS:
        assert np.isfinite(r[k]).all(), (what, k)


# ---------------------------------------------------------------------------------------------- the inputs
class Input:
    """a model, an alignment (with its mask table), the reference's mapping of it, and how many sites the oracle loses"""

    def __init__(self, args, aln, masks=None, ops=None, reference=True):
        self.args, self.aln, self.masks = args, np.ascontiguousarray(aln), masks
        self.om = oracle.Model(*args)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.lost = int(np.isinf(oracle.map_sites(self.om, self.aln, masks)["logL"]).sum())
        parent, blen, lot, Q, pi, rates, probs = args
        self.ref = sr.map_sites(parent, blen, lot, self.aln, Q, pi, rates, probs, masks=masks, ops=ops) if reference else None

    def engine(self):
        eng = engine.Engine(*self.args)
        eng.set_likelihood_scaling(True)
        return eng


def _model(S):
    return pm.synthetic_reversible(S, 161) + tuple(np.asarray(x) for x in pm.gamma_rates(0.5, 4))


def _long_tree():
    parent, blen, lot = synthetic.random_tree(300, 77)
    return parent, blen * 25.0, lot


@lru_cache(maxsize=None)
def long21():
    args = _long_tree() + _model(21)
    aln = oracle.simulate(oracle.Model(*args), 78, 0, 40)[0]
    aln[5, ::6] = 21                                    # an unknown
    return Input(args, aln)


@lru_cache(maxsize=None)
def star21():
    parent = np.full(321, 320, dtype=np.int32)
    parent[-1] = -1
    blen = np.full(321, 2.0)
    blen[-1] = 0.0
    args = (parent, blen, np.arange(320, dtype=np.int32)) + _model(21)
    return Input(args, oracle.simulate(oracle.Model(*args), 78, 0, 8)[0])


def _protein_codes(aln):
    masks = oracle.default_masks(20)[:22].copy()
    masks[21] = (1 << 2) | (1 << 3)
    aln = aln.copy()
    aln[3, ::3] = 21
    aln[7, 1::2] = 20
    return aln, masks


@lru_cache(maxsize=None)
def protein_masks(nsites=8):
    case = sc.long(20, 300)
    sim = case.aln if nsites == 8 else oracle.simulate(case.om, 78, 0, nsites)[0]
    assert np.array_equal(sim[:, :8], case.aln)
    aln, masks = _protein_codes(sim)
    return Input(case.model_args(), aln, masks, ops=case.ops())


@lru_cache(maxsize=None)
def shared(name):
    """a case of tests/scaled_cases.py as it stands, with that module's cached reference"""
    case = {"long20x600": lambda: sc.long(20, 600), "star": sc.star, "multi": sc.multi}[name]()
    inp = Input(case.model_args(), case.aln, reference=False)
    inp.ref = case.reference()
    return inp


INPUTS = {"long21": long21, "star21": star21, "protein_masks": protein_masks, "long20x600": lambda: shared("long20x600"),
          "star": lambda: shared("star"), "multi": lambda: shared("multi")}


def _both(eng, aln, masks=None):
    with scaled_plain(False):
        new = eng.map_sites(aln, masks)
    with scaled_plain(True):
        plain = eng.map_sites(aln, masks)
    return new, plain


# ---------------------------------------------------------------------------------------------- 1. paths and parity
@pytest.mark.parametrize("name", list(INPUTS))
def test_both_paths_meet_the_reference_and_each_other(name):
    inp = INPUTS[name]()
    assert inp.lost >= 2                                # the unscaled computation loses sites here
    eng = inp.engine()
    new, plain = _both(eng, inp.aln, inp.masks)
    _finite(new, "new")
    _finite(plain, "plain")
    _check_plain(new, inp.ref)
    _check_plain(plain, inp.ref)
    _check_plain(new, plain)
    assert new["counts"].tobytes() != plain["counts"].tobytes()   # sums in two orders: the switch did choose the kernels


# ---------------------------------------------------------------------------------------------- 2. 61 states under underflow
def test_61_states_where_fp64_underflows():
    """the long21 tree at 61 states, 8 sites of seed 78: 4 of them are lost in the C oracle.  Building that oracle model takes
    longer than the rest of this file, so the precondition is asserted on the engine's own unscaled mapping, and the
    columns come from the engine's simulator (pinned to the oracle's by tests/test_gpu_parity.py)"""
    eng = engine.Engine(*(_long_tree() + _model(61)))
    aln, _ = eng.simulate(78, 0, 8)
    with np.errstate(invalid="ignore"):
        assert np.isinf(eng.map_sites(aln)["logL"]).sum() >= 2
    eng.set_likelihood_scaling(True)
    new, plain = _both(eng, aln)
    _finite(new, "new")
    _finite(plain, "plain")
    _check_plain(new, plain)
    assert new["counts"].tobytes() != plain["counts"].tobytes()


# ---------------------------------------------------------------------------------------------- 3. nothing underflows
def _small(name):
    if name == "protein12_masks":
        case, masks = _masked_protein_case()
        return case, masks
    return _case(int(name)), None


def _args(case):
    return (case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])


@pytest.mark.parametrize("name", ["61", "64", "21", "7", "2", "protein12_masks"])
def test_scaled_matches_the_oracle_and_the_unscaled_call(name):
    case, masks = _small(name)
    eng = engine.Engine(*_args(case))
    o = oracle.map_sites(oracle.Model(*_args(case)), case["aln"], masks)
    assert np.isfinite(o["logL"]).all()
    off = eng.map_sites(case["aln"], masks)
    eng.set_likelihood_scaling(True)
    with scaled_plain(False):
        on = eng.map_sites(case["aln"], masks)
    _check_plain(on, o)
    _check_plain(on, off)
    assert (on["counts"] >= 0).all()


@pytest.mark.parametrize("name", ["61", "protein12_masks"])
def test_two_count_types_under_scaling(name):
    case, masks = _small(name)
    Bk = _two_types(case["Q"])
    eng = engine.Engine(*_args(case), Bk=Bk)
    assert eng.K == 2
    o = oracle.map_sites(oracle.Model(*_args(case), Bk=Bk), case["aln"], masks)
    eng.set_likelihood_scaling(True)
    with scaled_plain(False):
        on = eng.map_sites(case["aln"], masks)
    assert on["counts"].shape == (case["aln"].shape[1], eng.B, 2)
    _check_plain(on, o)


@pytest.mark.parametrize("name", ["61", "protein12_masks"])
def test_signed_weighted_register_under_scaling(name):
    case, masks = _small(name)
    S = len(case["pi"])
    W = np.random.default_rng(3).uniform(0.0, 2.0, size=(S, S))
    Bw = synthetic.weighted_register(case["Q"], W - W.mean())[None]
    eng = engine.Engine(*_args(case), Bk=Bw, clamp_negative=False)
    o = oracle.map_sites(oracle.Model(*_args(case), Bk=Bw, nonneg=False), case["aln"], masks)
    assert (o["counts"] < 0).any() and (o["counts"] > 0).any()
    eng.set_likelihood_scaling(True)
    with scaled_plain(False):
        r = eng.map_sites(case["aln"], masks)
    atol = 1e-12 * np.abs(o["counts"]).max()            # signed counts cancel: absolute, on the scale of the call
    rel_close(r["counts"], o["counts"], 1e-9, atol)
    rel_close(r["norm"], o["norm"], 1e-9, atol)
    rel_close(r["logL"], o["logL"], 1e-12)
    rel_close(r["post_rate"], o["post_rate"], 1e-12)
    assert np.array_equal(r["rate_class"], o["rate_class"])


# ---------------------------------------------------------------------------------------------- 4. tiles
@pytest.fixture(scope="module", params=["long21", "protein_masks"])
def tiles(request):
    inp = long21() if request.param == "long21" else protein_masks(17)
    eng = inp.engine()
    with scaled_plain(False):
        full = eng.map_sites(inp.aln, inp.masks)
    _finite(full)
    return request.param, inp, eng, full


def test_a_sites_bytes_do_not_depend_on_the_call(tiles):
    name, inp, eng, full = tiles
    for n in ((1, 15, 16, 17, 33, 40) if name == "long21" else (1, 8, 17)):
        r = eng.map_sites(inp.aln[:, :n], inp.masks)
        _same_bytes(r, {k: full[k][:n] for k in KEYS}, n)


def test_reversed_columns_repeated_calls_and_calls_without_counts(tiles):
    _, inp, eng, full = tiles
    _same_bytes(eng.map_sites(inp.aln, inp.masks), full, "repeat")
    rev = eng.map_sites(np.ascontiguousarray(inp.aln[:, ::-1]), inp.masks)
    _same_bytes(rev, {k: np.ascontiguousarray(full[k][::-1]) for k in KEYS}, "reversed")
    bare = eng.map_sites(inp.aln, inp.masks, want_counts=False)
    assert bare["counts"] is None
    _same_bytes(bare, full, "no counts", KEYS[1:])


def test_a_tile_that_mixes_resolved_and_unknown_symbols_at_a_leaf():
    inp = long21()
    cols = np.array([j for j in range(20) if j % 6][:16])
    assert len(cols) == 16 and (inp.aln[:, cols] < 21).all() and (inp.aln[5, :16] == 21).any() and (inp.aln[5, :16] < 21).any()
    eng = inp.engine()
    mixed = eng.map_sites(inp.aln)                      # tile 0: leaf 5 holds unknowns and states
    resolved = eng.map_sites(np.ascontiguousarray(inp.aln[:, cols]))   # one tile, every leaf resolved
    _same_bytes(resolved, {k: mixed[k][cols] for k in KEYS})


# ---------------------------------------------------------------------------------------------- 5. tree shapes
@pytest.mark.parametrize("S", [61, 20])
@pytest.mark.parametrize("name", ["(x,x)", "(x,x,x)", "((x,x),(x,x))", "five", "caterpillar12"])
def test_tree_shapes_under_scaling_match_the_oracle(name, S):
    parent, lot = _shape(name)
    rng = np.random.default_rng(len(parent))
    blen = rng.uniform(0.03, 0.5, size=len(parent))
    blen[-1] = 0.0
    if S == 20:
        mdl = synthetic.protein_model(0.5, 4)
        model = (mdl["Q"], mdl["pi"], mdl["rates"], mdl["probs"])
    else:
        model = _model(S)
    eng = engine.Engine(parent, blen, lot, *model)
    om = oracle.Model(parent, blen, lot, *model)
    aln, _ = oracle.simulate(om, 11, 0, 20)
    aln[0, ::6] = S                                     # an unknown
    eng.set_likelihood_scaling(True)
    with scaled_plain(False):
        _check_plain(eng.map_sites(aln), oracle.map_sites(om, aln))


# ---------------------------------------------------------------------------------------------- 6. model sets
def test_model_sets_under_scaling_match_the_oracle():
    c = ms.case("c61x2")
    mob = (c["mob"] % 2).astype(np.int32)               # two of the case's generators
    eng = engine.Engine(c["parent"], c["blen"], c["lot"], c["Qs"], c["pis"], c["rates"], c["probs"], model_of_branch=mob,
                        root_freqs=c["root"])
    aln = ms.alignment(c, 70, ambiguous=True)
    eng.set_likelihood_scaling(True)
    with scaled_plain(False):
        _check_plain(eng.map_sites(aln), oracle.map_sites(ms.oracle_of(c, mob=mob), aln))
    c = ms.case("p20x4")
    eng, aln = ms.engine_of(c), ms.alignment(c, 70)
    eng.set_likelihood_scaling(True)
    with scaled_plain(False):
        _check_plain(eng.map_sites(aln), oracle.map_sites(ms.oracle_of(c), aln))


# ---------------------------------------------------------------------------------------------- 7. untouched neighbours
@pytest.mark.parametrize("name", ["c61", "protein", "dna"])
def test_neighbours_ignore_the_switch(name):
    if name == "c61":
        case = _case(61, nsites=40)
    else:
        case = make_case(12, 40, 20, 77) if name == "protein" else make_case(14, 40, 4, 31)
    eng = engine.Engine(*_args(case))
    got = []
    for on in (False, True):
        out = []
        with scaled_plain(on):
            try:
                out += [eng.map_sites(case["aln"])[k] for k in KEYS]       # every unscaled mapping
                for average, joint in sc.OPTIONS[1:]:
                    eng.set_mapping_options(average, joint)
                    out += [eng.map_sites(case["aln"])[k] for k in KEYS]
                eng.set_likelihood_scaling(True)
                for average, joint in sc.OPTIONS[1:]:                       # the three other options, scaled
                    eng.set_mapping_options(average, joint)
                    out += [eng.map_sites(case["aln"])[k] for k in KEYS]
                eng.set_mapping_options(True, True)
                a = eng.ancestral_states(case["aln"], want_posterior=True)  # scaled ancestral states
                out += [a["states"], a["post"]]
                if name == "dna":                                           # the scaled mapping at 4 states
                    out += [eng.map_sites(case["aln"])[k] for k in KEYS]
            finally:
                eng.set_likelihood_scaling(False)
                eng.set_mapping_options(True, True)
        got.append(out)
    assert len(got[0]) == len(got[1]) == (42 if name == "dna" else 37)
    for i, (a, b) in enumerate(zip(*got)):
        assert a.tobytes() == b.tobytes(), i


def test_the_wide_switch_does_not_touch_scaled_calls():
    inp = long21()
    eng = inp.engine()
    was = engine.map_wide_plain(False)
    try:
        a = eng.map_sites(inp.aln)
        engine.map_wide_plain(True)
        b = eng.map_sites(inp.aln)
    finally:
        engine.map_wide_plain(was)
    _same_bytes(a, b)


# ---------------------------------------------------------------------------------------------- 8. pipelines
def test_null_intra_agrees_between_the_two_paths():
    eng = sc.long(20, 300).engine()
    eng.set_likelihood_scaling(True)
    with scaled_plain(False):
        new = eng.null_intra(engine.STAT_CORRELATION, 5, 0, 3, 8)
    with scaled_plain(True):
        plain = eng.null_intra(engine.STAT_CORRELATION, 5, 0, 3, 8)
    for k in new:
        assert not np.isnan(new[k]).any(), k
    rel_close(new["stat"], plain["stat"], 1e-6, 1e-12)
    rel_close(new["nmin"], plain["nmin"], 1e-9)
    assert np.array_equal(new["rcmin"], plain["rcmin"])


def test_observed_mapping_on_a_side_stream_beside_the_null():
    """test_gpu_two_streams' pattern: the serial run is the reference, three overlapped runs give the same bytes.  Not under
    the scratch guard, which synchronises at every scratch request."""
    import torch
    was = engine.scratch_guard(False)
    try:
        case = sc.long(20, 300)
        eng = case.engine()
        eng.set_likelihood_scaling(True)
        dev = torch.device("cuda:0")
        d_aln = torch.from_numpy(case.aln).to(dev)
        n, nrep, ram = case.aln.shape[1], 3, 8
        f64 = dict(dtype=torch.float64, device=dev)

        def run(overlap):
            obs = dict(counts=torch.zeros(eng.B * eng.K, n, **f64), logL=torch.zeros(n, **f64), post_rate=torch.zeros(n, **f64),
                       rate_class=torch.zeros(n, dtype=torch.int32, device=dev), norm=torch.zeros(n, **f64))
            nul = dict(stat=torch.zeros(nrep * ram, **f64), rcmin=torch.zeros(nrep * ram, dtype=torch.int32, device=dev),
                       prmin=torch.zeros(nrep * ram, **f64), nmin=torch.zeros(nrep * ram, **f64))
            side = torch.cuda.Stream(device=dev)
            torch.cuda.synchronize()
            if overlap:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    eng.map_sites_dev(d_aln, **obs)
                eng.null_intra_dev(engine.STAT_CORRELATION, 9, 0, nrep, ram, **nul)
                torch.cuda.current_stream().wait_stream(side)
            else:
                eng.map_sites_dev(d_aln, **obs)
                torch.cuda.synchronize()
                eng.null_intra_dev(engine.STAT_CORRELATION, 9, 0, nrep, ram, **nul)
            torch.cuda.synchronize()
            return [t.cpu().numpy() for t in list(obs.values()) + list(nul.values())]

        with scaled_plain(False):
            seq = run(False)
            assert np.isfinite(seq[-4]).all() and np.isfinite(seq[0]).all()
            for k in range(3):
                for i, (a, b) in enumerate(zip(seq, run(True))):
                    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (k, i)
        eng.close()
    finally:
        engine.scratch_guard(was)


# ---------------------------------------------------------------------------------------------- 9. the scratch guard
def test_new_path_under_the_scratch_guard():
    l21, pmk = long21(), protein_masks()
    was = engine.scratch_guard(True)
    engine.scratch_guard_failures(clear=True)
    try:
        with scaled_plain(False):
            e1, e2 = l21.engine(), pmk.engine()         # the guard holds for contexts created from now on
            for n in (40, 17):
                r = e1.map_sites(l21.aln[:, :n])
                _check_plain(r, {k: l21.ref[k][:n] for k in KEYS})
            _check_plain(e2.map_sites(pmk.aln, pmk.masks), pmk.ref)
            for e in (e1, e2):
                e.synchronize()                         # verifies every canary of the context
                e.scratch_check()
        assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()
        e1.close()
        e2.close()
    finally:
        engine.scratch_guard(was)
