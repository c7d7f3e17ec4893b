"""-m gpu: the default mapping of alphabets other than 4 / 20 states on the f64 matrix instruction (cmx_map_wide.hip).

Such a context pads its states to 64 and maps through the plain stage's passes; by default the default mapping
(nijt.average = yes, nijt.joint = yes) and the site scalars now run matrix-core kernels, 16 sites of one rate class per
wave, and cmx_debug_map_wide_plain(1) forces the plain kernels the variants use.  Here: the switch; both paths against
the oracle (generic in the state count) and against each other; partial tiles, a tile across the row stride, bytes that
depend on a site's column alone; tree shapes; a model set and signed weights; the kernels this change must leave alone,
as bytes; the null pipeline and the two-stream use.  Tolerances are those of
test_gpu_codon_alphabets.test_plain_alphabet_mapping_matches_oracle unless a test says otherwise."""
import numpy as np
import pytest

import model_sets as ms
import oracle
from comap_amd import engine, protein_models as pm, synthetic
from conftest import rel_close
from test_gpu_codon_alphabets import _case, _pair
from tree_shapes import _caterpillar, by_name, rooted_catalogue

pytestmark = pytest.mark.gpu

KEYS = ("counts", "logL", "post_rate", "rate_class", "norm")


class forced_plain:
    """with forced_plain(on): the switch set for the block, the previous state back afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = engine.map_wide_plain(self.on)

    def __exit__(self, *exc):
        engine.map_wide_plain(self.was)


def _check(r, o, atol=1e-300):
    rel_close(r["counts"], o["counts"], 1e-9, atol)
    rel_close(r["logL"], o["logL"], 1e-12)
    rel_close(r["post_rate"], o["post_rate"], 1e-12)
    rel_close(r["norm"], o["norm"], 1e-9, 0.0 if atol == 1e-300 else atol)
    assert np.array_equal(r["rate_class"], o["rate_class"])


def _same_bytes(a, b, what=""):
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---------------------------------------------------------------------------------------------- 1. the switch
def test_switch_defaults_to_off_and_round_trips():
    was = engine.map_wide_plain(None)
    try:
        assert was is False
        assert engine.map_wide_plain(True) is False
        assert engine.map_wide_plain(None) is True
        assert engine.map_wide_plain(False) is True
        assert engine.map_wide_plain(None) is False
    finally:
        engine.map_wide_plain(was)


# ---------------------------------------------------------------------------------------------- 2. parity
def _two_types(Q):
    B0 = synthetic.weighted_register(Q)
    S = len(B0)
    ts = np.triu(np.ones((S, S)), 1)
    ts = ts + ts.T
    ts[:, ::2] = 0                                      # type 0 = into odd states, type 1 = the rest
    return np.stack([B0 * ts, B0 * (1 - ts)])


@pytest.mark.parametrize("S,K", [(61, 1), (64, 1), (21, 1), (7, 1), (2, 1), (61, 2)])
def test_both_paths_match_the_oracle_and_each_other(S, K):
    case = _case(S)                                     # 9 taxa, 70 sites (four tiles of 16 and one of 6), Gamma 4, unknowns S and 200
    kw = dict(Bk=_two_types(case["Q"])) if K == 2 else {}
    eng = engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"], **kw)
    om = oracle.Model(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"], **kw)
    assert eng.info()["nstates"] == S and eng.K == K
    o = oracle.map_sites(om, case["aln"])
    with forced_plain(False):
        wide = eng.map_sites(case["aln"])
    with forced_plain(True):
        plain = eng.map_sites(case["aln"])
    assert wide["counts"].shape == (70, eng.B, K)
    _check(wide, o)
    _check(plain, o)
    _check(wide, plain)
    assert (wide["counts"] >= 0).all() and (plain["counts"] >= 0).all()
    if S == 61:                                         # 61-term sums in two orders: the switch did choose the kernels
        assert wide["counts"].tobytes() != plain["counts"].tobytes()


# ---------------------------------------------------------------------------------------------- 3. tiles
@pytest.fixture(scope="module")
def tiles():
    case = _case(61, nsites=300)
    eng, _ = _pair(case)
    return case, eng, eng.map_sites(case["aln"])        # 300 sites: chunk = 300, a tile straddles the row stride


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 300])
def test_a_sites_bytes_do_not_depend_on_the_call(tiles, n):
    case, eng, full = tiles
    r = eng.map_sites(case["aln"][:, :n])
    _same_bytes(r, {k: full[k][:n] for k in KEYS}, n)
    assert np.isfinite(r["counts"]).all() and np.isfinite(r["logL"]).all()


def test_reversed_columns_give_reversed_bytes_and_calls_repeat(tiles):
    case, eng, full = tiles
    _same_bytes(eng.map_sites(case["aln"]), full, "repeat")
    rev = eng.map_sites(np.ascontiguousarray(case["aln"][:, ::-1]))
    _same_bytes(rev, {k: np.ascontiguousarray(full[k][::-1]) for k in KEYS}, "reversed")


def test_partial_tiles_under_the_scratch_guard(tiles):
    case, _, full = tiles
    was = engine.scratch_guard(True)
    engine.scratch_guard_failures(clear=True)
    engine.scratch_shrink(None, 0)
    try:
        eng, _ = _pair(case)                            # the guard holds for contexts created from now on
        for n in (300, 17):
            _same_bytes(eng.map_sites(case["aln"][:, :n]), {k: full[k][:n] for k in KEYS}, n)
            eng.synchronize()                           # verifies every canary of the context
            eng.scratch_check()
        assert engine.scratch_guard_failures() == [], engine.scratch_guard_failures()
        eng.close()
    finally:
        engine.scratch_shrink(None, 0)
        engine.scratch_guard(was)


# ---------------------------------------------------------------------------------------------- 4. tree shapes
def _five_children():
    """five leaves under one node, that node and a sixth leaf under the root"""
    return np.array([5, 5, 5, 5, 5, 7, 7, -1], dtype=np.int32), np.array([0, 1, 2, 3, 4, 6], dtype=np.int32)


def _shape(name):
    if name == "five":
        return _five_children()
    if name == "caterpillar12":
        return _caterpillar(12)
    sh = by_name(name, rooted_catalogue(2, 4))
    return sh.parent, sh.lot


@pytest.mark.parametrize("name", ["(x,x)", "(x,x,x)", "((x,x),(x,x))", "five", "caterpillar12"])
def test_tree_shapes_match_the_oracle(name):
    parent, lot = _shape(name)
    rng = np.random.default_rng(len(parent))
    blen = rng.uniform(0.03, 0.5, size=len(parent))
    blen[-1] = 0.0
    Q, pi = pm.synthetic_reversible(61, 161)
    rates, probs = pm.gamma_rates(0.5, 4)
    eng = engine.Engine(parent, blen, lot, Q, pi, rates, probs)
    om = oracle.Model(parent, blen, lot, Q, pi, rates, probs)
    aln, _ = oracle.simulate(om, 11, 0, 20)
    aln[0, ::6] = 61                                    # an unknown
    _check(eng.map_sites(aln), oracle.map_sites(om, aln))


# ---------------------------------------------------------------------------------------------- 5. model sets, signed weights
def test_two_model_set_with_root_frequencies_matches_the_oracle():
    c = ms.case("c61x2")
    mob = (c["mob"] % 2).astype(np.int32)               # two of the case's generators
    eng = engine.Engine(c["parent"], c["blen"], c["lot"], c["Qs"], c["pis"], c["rates"], c["probs"], model_of_branch=mob,
                        root_freqs=c["root"])
    aln = ms.alignment(c, 70, ambiguous=True)
    _check(eng.map_sites(aln), oracle.map_sites(ms.oracle_of(c, mob=mob), aln))


def test_signed_weighted_register_matches_the_oracle():
    case = _case(61)
    W = np.random.default_rng(3).uniform(0.0, 2.0, size=(61, 61))
    Bw = synthetic.weighted_register(case["Q"], W - W.mean())[None]
    args = (case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])
    r = engine.Engine(*args, Bk=Bw, clamp_negative=False).map_sites(case["aln"])
    o = oracle.map_sites(oracle.Model(*args, Bk=Bw, nonneg=False), case["aln"])
    assert (o["counts"] < 0).any() and (o["counts"] > 0).any()
    _check(r, o, atol=1e-12 * np.abs(o["counts"]).max())   # signed counts cancel: absolute, on the scale of the call


# ---------------------------------------------------------------------------------------------- 6. untouched neighbours
def test_variants_ancestral_states_and_scaled_mapping_ignore_the_switch():
    case = _case(61, nsites=40)
    eng, _ = _pair(case)
    got = []
    for on in (False, True):
        out = []
        with forced_plain(on):
            try:
                for average, joint in ((False, True), (True, False), (False, False)):
                    eng.set_mapping_options(average, joint)
                    out += [eng.map_sites(case["aln"])[k] for k in KEYS]
                eng.set_mapping_options(True, True)
                a = eng.ancestral_states(case["aln"], want_posterior=True)
                out += [a["states"], a["post"]]
                eng.set_likelihood_scaling(True)
                out += [eng.map_sites(case["aln"])[k] for k in KEYS]
            finally:
                eng.set_likelihood_scaling(False)
                eng.set_mapping_options(True, True)
        got.append(out)
    assert len(got[0]) == len(got[1]) == 22
    for i, (a, b) in enumerate(zip(*got)):
        assert a.tobytes() == b.tobytes(), i


# ---------------------------------------------------------------------------------------------- 7. pipelines
def test_null_intra_agrees_between_the_two_paths():
    case = _case(61)
    eng, _ = _pair(case)
    with forced_plain(False):
        wide = eng.null_intra(engine.STAT_CORRELATION, 11, 0, 3, 40)
    with forced_plain(True):
        plain = eng.null_intra(engine.STAT_CORRELATION, 11, 0, 3, 40)
    rel_close(wide["stat"], plain["stat"], 1e-6, 1e-12)
    rel_close(wide["nmin"], plain["nmin"], 1e-9)


def test_observed_mapping_on_a_side_stream_beside_the_null():
    """test_gpu_two_streams' pattern: the serial run is the reference, three overlapped runs give the same bytes.  Not under
    the scratch guard, which synchronises at every scratch request."""
    import torch
    was = engine.scratch_guard(False)
    try:
        case = _case(61, nsites=2000)
        eng, _ = _pair(case)
        dev = torch.device("cuda:0")
        d_aln = torch.from_numpy(case["aln"]).to(dev)
        n, nrep, ram = 2000, 3, 200
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

        seq = run(False)
        assert np.isfinite(seq[-4]).any() and np.isfinite(seq[0]).all()
        for k in range(3):
            for i, (a, b) in enumerate(zip(seq, run(True))):
                assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (k, i)
        eng.close()
    finally:
        engine.scratch_guard(was)
