"""-m gpu: what a call returns does not depend on what its context did before.

An integrator keeps one cmx_ctx per GPU for a whole analysis and sends every entry point through it in whatever order
the option file dictates.  The context caches a lot lazily ("Context state"): the leaf operators' ambiguity
rows, kept Gram blocks, statistic weights, mapping / null options, operators uploaded at first use, the permutation
test's table, eight rotating parameter slots and some 140 named grow-only scratch buffers that unrelated entry points
share.  Here three contexts (20 states, 4 states, a codon-sized plain alphabet) stay alive for the whole module and a
catalogue of ops (tests/context_history_plan.py names them, the closures are below) runs on them

  * along a walk that makes every ordered pair of a context's ops neighbours (N * N steps, default settings),
  * along seeded random histories over all three contexts with the setting ops mixed in,
  * and along one such history per alphabet under the scratch guard (reuse of a grown buffer at a smaller logical size
    is where an overrun hides in allocator slack).

Reference of a step: the same op with the same settings on a fresh Engine of the same model that has done nothing else.
Same library, same inputs, same launch shapes: np.array_equal(.., equal_nan=True), no tolerance.  So that this is not
a circular anchor, every op's fresh result at the default settings is compared once with the oracle at the tolerance of
the existing parity test of that entry point (tests/test_gpu_parity.py, test_gpu_cluster.py, test_gpu_candidates.py,
test_gpu_mi_bounds.py, test_gpu_ancestral.py, test_gpu_codon_alphabets.py); no tolerance is new here.

Ops that need not be byte-reproducible (NOT_BYTE_REPRODUCIBLE): mi_columns_unknowns_* and mi_pairs_unknowns_*.
mi_columns_kernel / mi_pairs_kernel add the fractional weights of ambiguous letters with floating-point atomicAdd
(comap_amd/csrc/cmx_mica.hip, `atomicAdd(&joint[...], w)` in both kernels), so the order of the additions, and with
it the last bits, may differ from run to run.  These ops stay in every sequence and are compared with the oracle, at
the tolerance of test_mi_columns_matches_oracle_with_ambiguity, at every step instead.  Every other op must be equal
byte for byte on two fresh contexts (first test) -- a difference there is a finding, not an exception.

The compact_* ops also assert, inside the op, that the records made from kept Gram blocks equal the records the same
context computes without kept blocks right afterwards: stale kept blocks (other weights, rewritten vectors) would be
equally stale on a fresh context, so fresh-versus-history alone could not see them."""
import time

import numpy as np
import pytest

import context_history_plan as plan
import oracle
import weighted_reference as wr
from oracle import candidates as ocand
from oracle import cluster as oc
from comap_amd import engine, protein_models as pm, synthetic
from conftest import make_case, rel_close

pytestmark = pytest.mark.gpu

NOT_BYTE_REPRODUCIBLE = {"mi_columns_unknowns_s", "mi_columns_unknowns_l", "mi_pairs_unknowns_s", "mi_pairs_unknowns_l"}
BOUNDS = np.array([0.0, 1e-4, 1e-3, 1e-3, 0.01, 0.05, 0.3, 1.0, 50.0, 1e4])
NCLS = 6
FILTERS = dict(min_rate_class=1, max_rate_class_diff=1, min_rate=0.3, max_rate_diff=1.5, min_statistic=0.2)


# ------------------------------------------------------------------------------------------------ inputs
class Inputs:
    """everything an op reads, made once per context from the oracle (never from the engine under test)"""

    def __init__(self, name):
        self.name = name
        seed = {"p20": 811, "n4": 812, "c61": 813}[name]
        rng = np.random.default_rng(seed)
        if name == "p20":
            case, self.A = make_case(10, 130, 20, seed), 20
        elif name == "n4":
            case, self.A = make_case(12, 150, 4, seed), 4
        else:
            case, self.A = make_case(6, 30, 20, seed), 0      # (61 states: the oracle is slow, everything is smaller here)
            Q, pi = pm.synthetic_reversible(61, seed + 100)
            aln = rng.integers(0, 61, size=case["aln"].shape).astype(np.uint8)
            base = rng.integers(0, 61, size=(1, aln.shape[1]))
            aln = np.where(rng.random(aln.shape) < 0.6, base, aln).astype(np.uint8)
            aln[2, ::7] = 61
            aln[5, 3::11] = 200
            case.update(Q=Q, pi=pi, aln=aln)
        self.case = case
        self.S = len(case["pi"])
        self.om = self._omodel(case)
        c2 = dict(case)
        c2["blen"] = case["blen"] * rng.uniform(0.5, 1.5, size=len(case["blen"]))
        m2 = synthetic.dna_model(0.9, 3) if name == "n4" else synthetic.protein_model(0.9, 3)
        c2.update(rates=m2["rates"], probs=m2["probs"])
        self.case2, self.om2 = c2, self._omodel(c2)
        self.aln = case["aln"]
        self.T, self.NL = self.aln.shape
        self.n = {"s": 3, "l": self.NL}            # sites of the pair / rows / group ops
        self.nmap = {"s": 1, "l": self.NL}         # sites of the mapping ops
        self.m = oracle.map_sites(self.om, self.aln)
        self.counts = self.m["counts"]
        self.B = self.counts.shape[1]
        self.aln2 = np.ascontiguousarray(self.aln[:, ::-1])
        self.n2 = {"s": 2, "l": min(77, self.NL - 7)}
        self.m2 = oracle.map_sites(self.om, self.aln2)
        self.counts2 = self.m2["counts"][:self.n2["l"]]
        # ambiguity codes (about 15 %) and their table
        if name == "n4":
            self.masks = np.array([1, 2, 4, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15, 15], dtype=np.uint32)
            ncodes = 12
        elif name == "p20":
            self.masks = oracle.default_masks(20)[:24].copy()
            self.masks[20], self.masks[21] = (1 << 2) | (1 << 3), (1 << 5) | (1 << 6)
            ncodes = 4
        else:
            self.masks, ncodes = None, 0
        if ncodes:
            hit = rng.random(self.aln.shape) < 0.15
            self.aln_amb = self.aln.copy()
            self.aln_amb[hit] = rng.integers(self.S, self.S + ncodes, size=int(hit.sum()), dtype=np.uint8)
        self.w = {"a": rng.uniform(0.2, 2.0, size=self.B), "b": rng.uniform(0.2, 2.0, size=self.B)}
        base_mv = self.counts.sum(axis=2).mean(axis=0)
        self.mv = [base_mv * (0.5 + 0.1 * i) + 0.01 * i for i in range(11)]
        self.stat = oracle.pair_stats_intra(0, self.counts)
        plain = name == "c61"
        self.null = oracle.null_intra(self.om, 0, 99, 0, 4 if plain else 10, 15 if plain else 50)
        # (replicates, sites per replicate): 150 null pairs, not whole 64-site blocks
        self.nrep = {"s": (1, 5), "l": (2, 13) if plain else (3, 50)}
        self.cluster_null = {"s": (0, 1, 5), "l": (1, 3, 12) if plain else (2, 5, 40)}
        self.sup = {sz: np.stack([np.stack([oracle.simulate(self.om, 5, (r * 2 + h) * ram, ram)[0] for h in range(2)])
                                  for r in range(nr)]) for sz, (nr, ram) in self.nrep.items()}
        self.groups = {"s": [[0, 1], [0, 1, 2]],
                       "l": [list(rng.choice(self.NL, size=min(int(k), self.NL - 3), replace=False)) for k in (2, 3, 5, 12, 2, 40)]}
        self.cand = {}
        for sz, ng in (("s", 1), ("l", 5)):
            n = self.n[sz]
            gs = [list(rng.choice(n, size=int(rng.integers(2, min(5, n + 1))), replace=False)) for _ in range(ng)]
            win = [[(self.m["norm"][i] - 0.3, self.m["norm"][i] + 0.3) for i in g] for g in gs]
            obs = np.array([ocand.group_stat(0, [self.counts[i] for i in g], oracle.stat_params(0)) for g in gs])
            args = dict(min_sim=3, rep_ram=8, max_trials=2, seed=2024, max_batches=20) if sz == "s" else \
                dict(min_sim=25, rep_ram=16 if plain else 48, max_trials=4, seed=2024, max_batches=4 if plain else 60)
            self.cand[sz] = (win, [1] * ng, obs, args)
        x = rng.normal(size=(90, 5))
        d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
        d = (d + d.T) / 2
        np.fill_diagonal(d, 0.0)
        self.dist = {"s": d[:3, :3].copy(), "l": d}
        if self.A:
            A, Tm = self.A, 40
            core = rng.integers(0, A, size=(Tm, 1))
            self.mica1 = np.where(rng.random((Tm, 70)) < 0.5, core, rng.integers(0, A, size=(Tm, 70))).astype(np.uint8)
            self.mica2 = rng.integers(0, min(A, 6), size=(Tm, 33)).astype(np.uint8)
            self.mica1u, self.mica2u = self.mica1.copy(), self.mica2.copy()
            self.mica1u[rng.random(self.mica1.shape) < 0.05] = A + 2              # an unknown
            self.mica2u[rng.random(self.mica2.shape) < 0.05] = A                  # a partial code: two states
            self.mica_masks = oracle.default_masks(A)
            self.mica_masks[A] = (1 << 3) | (1 << 2)
            self.mica_n = {"s": (3, 2), "l": (70, 33)}
            self.mica_idx = {sz: (rng.integers(0, n1, size=k), rng.integers(0, n2, size=k))
                             for sz, (n1, n2), k in (("s", self.mica_n["s"], 4), ("l", self.mica_n["l"], 111))}
            self.mica_o = oracle.mi_columns(self.mica1, self.mica1, A)
            self.perm = {}
            for Tp in (30, 64):    # coupled columns with two unknown codes sprinkled in; three columns stay resolved
                core = rng.integers(0, A, size=(Tp, 1))
                a = np.where(rng.random((Tp, 9)) < 0.55, core, rng.integers(0, A, size=(Tp, 9))).astype(np.uint8)
                hit = rng.random((Tp, 9)) < 0.2
                hit[:, :3] = False
                a[hit] = rng.integers(A, A + 2, size=int(hit.sum()))
                self.perm[Tp] = a
        self._oracle = {}

    @staticmethod
    def _omodel(case):
        return oracle.Model(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])

    @staticmethod
    def _engine(case):
        return engine.Engine(case["parent"], case["blen"], case["lot"], case["Q"], case["pi"], case["rates"], case["probs"])

    def site_scalars(self, n, m=None):
        m = self.m if m is None else m
        return dict(counts=m["counts"][:n], rate_class=m["rate_class"][:n], post_rate=m["post_rate"][:n], norm=m["norm"][:n])


class Ctx:
    """one context of the model of `inputs` (the second data set's engine is made when an op first asks for it) and the
    shadow record of its settings"""

    def __init__(self, inputs):
        self.I = inputs
        self.eng = Inputs._engine(inputs.case)
        self._eng2 = None
        self.settings = plan.Settings()

    @property
    def eng2(self):
        if self._eng2 is None:
            self._eng2 = Inputs._engine(self.I.case2)
        return self._eng2

    def set(self, op):
        plan.issue_setting(self.eng, op, self.I.w)
        self.settings.record(op)

    def weights(self):
        return None if self.settings.weights is None else self.I.w[self.settings.weights]

    def close(self):
        self.eng.close()
        if self._eng2 is not None:
            self._eng2.close()


# ------------------------------------------------------------------------------------------------ the catalogue
def _dev(x, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def _split(name):
    return (name[:-2], name[-1]) if name.endswith(("_s", "_l")) else (name, None)


def _rows_dict(prefix, rows, count):
    out = {prefix + f: np.ascontiguousarray(rows[f]) for f in rows.dtype.names}
    out[prefix + "count"] = np.array([count])
    return out


def op_map(c, sz, masks=False, dev=False):
    I = c.I
    aln = np.ascontiguousarray((I.aln_amb if masks else I.aln)[:, :I.nmap[sz]])
    if not dev:
        return c.eng.map_sites(aln, masks=I.masks if masks else None)
    import torch
    n, BK = aln.shape[1], c.eng.B * c.eng.K
    out = dict(counts=torch.zeros(BK, n, dtype=torch.float64, device="cuda"), logL=torch.zeros(n, dtype=torch.float64, device="cuda"),
               post_rate=torch.zeros(n, dtype=torch.float64, device="cuda"), rate_class=torch.zeros(n, dtype=torch.int32, device="cuda"),
               norm=torch.zeros(n, dtype=torch.float64, device="cuda"))
    c.eng.map_sites_dev(_dev(aln), **out)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["counts"] = np.ascontiguousarray(out["counts"].T).reshape(n, c.eng.B, c.eng.K)
    return out


def op_map_masks_refused(c, sz):
    I = c.I
    with pytest.raises(engine.CmxError) as e:
        c.eng.map_sites(I.aln[:, :5].copy(), masks=np.full(64, 0xFFFFFFFF, dtype=np.uint32))
    assert e.value.status == -3 or "ambiguity table" in str(e.value)
    return c.eng.map_sites(I.aln[:, :5].copy())          # a failed call leaves no state behind either


def op_asr(c, sz, masks=False):
    I = c.I
    aln = np.ascontiguousarray((I.aln_amb if masks else I.aln)[:, :I.nmap[sz]])
    mk = I.masks if masks else None
    r = c.eng.ancestral_states(aln, masks=mk, want_posterior=True)
    s = c.eng.ancestral_states(aln, masks=mk)
    return dict(states=r["states"], post=r["post"], states_alone=s["states"])


def op_simulate(c, sz):
    aln, cls = c.eng.simulate(43, 17, {"s": 1, "l": 300}[sz])
    return dict(aln=aln, cls=cls)


def op_simulate_continuous(c, sz):
    # (the oracle's continuous-rate simulator exponentiates a 61 x 61 generator per site and branch: fewer sites there)
    aln, rates = c.eng.simulate_continuous(44, 5, {"s": 1, "l": 70 if c.I.name == "c61" else 300}[sz], 0.7, 0.1)
    return dict(aln=aln, rates=rates)


def _pair_kw(I, kind, inter):
    if kind == 5:
        return dict(threshold=0.05)
    if kind == 6:
        return dict(mean_vectors=np.stack([I.mv[0], I.mv[1]]) if inter else I.mv[0])
    if kind == 8:
        return dict(threshold=BOUNDS)
    return {}


def op_pair(c, sz, kind):
    I = c.I
    n, n2 = I.n[sz], I.n2[sz]
    return dict(intra=c.eng.pair_stats(kind, I.counts[:n], **_pair_kw(I, kind, False)),
                inter=c.eng.pair_stats(kind, I.counts[:n], I.counts2[:n2], **_pair_kw(I, kind, True)))


def op_pair_k6_slots(c, sz):
    return {"mv%d" % i: c.eng.pair_stats(6, c.I.counts[:20], mean_vectors=c.I.mv[i]) for i in range(11)}


def op_null(c, sz, which):
    I = c.I
    nrep, ram = I.nrep[sz]
    if which == "fused":
        return c.eng.null_intra(0, 777, 0, nrep, ram)
    if which == "supplied":
        return c.eng.null_intra(1, 0, 0, nrep, ram, supplied=I.sup[sz])
    if which == "continuous":
        return c.eng.null_intra_continuous(0, 31, 0, nrep, ram, 0.7, 0.1)
    if which == "k6":
        return c.eng.null_intra(6, 13, 0, nrep, ram, mean_vectors=I.mv[2])
    if which == "bounds":
        return c.eng.null_intra(8, 15, 0, nrep, ram, threshold=BOUNDS)
    return c.eng.null_inter(c.eng2, 0, 4242, 1, 1 + nrep, ram)


def op_null_fused_patterns(c, sz, on):
    """the fused null under one value of cmx_set_null_patterns whatever the context's settings are: averaged joint
    mapping, no weights, that value; then the shadow settings go back.  null_pattern_count tells the paths apart: every
    simulated site with the patterns off, the distinct columns (never more) with them on."""
    nrep, ram = c.I.nrep[sz]
    eng = c.eng
    eng.set_mapping_options(True, True)
    eng.set_statistic_weights(None)
    eng.set_null_patterns(on)
    try:
        out = eng.null_intra(0, 777, 0, nrep, ram)
        mapped = eng.null_pattern_count()
    finally:
        plan.apply_settings(eng, c.settings, c.I.w)
    assert mapped == 2 * nrep * ram if on is False else 0 < mapped <= 2 * nrep * ram
    out["mapped"] = np.array([mapped])
    return out


def op_pvalues(c, sz):
    I = c.I
    n = I.n[sz]
    pv, ns = c.eng.intra_pvalues(I.stat[:n, :n].copy(), I.m["norm"][:n], NCLS, I.null["stat"], I.null["nmin"])
    return dict(pvalue=pv, nsim=ns)


def op_rows(c, sz):
    I = c.I
    n = I.n[sz]
    s = I.site_scalars(n)
    a = (0, s["counts"], s["rate_class"], s["post_rate"], s["norm"], I.null["stat"], I.null["nmin"], NCLS)
    out = _rows_dict("all_", *c.eng.intra_rows(*a))
    out.update(_rows_dict("filtered_", *c.eng.intra_rows(*a, filters=engine.PairFilters(**FILTERS))))
    out.update(_rows_dict("few_", *c.eng.intra_rows(*a, capacity=min(10, n * (n - 1) // 2 - 1))))
    return out


def op_inter_rows(c, sz):
    I = c.I
    m1, m2 = I.site_scalars(I.n[sz]), I.site_scalars(I.n2[sz], I.m2)
    out = _rows_dict("all_", *c.eng.inter_rows(0, m1, m2))
    out.update(_rows_dict("filtered_", *c.eng.inter_rows(0, m1, m2, filters=engine.InterFilters(min_statistic=0.1, max_rate_class_diff=1))))
    return out


def op_compact(c, sz, between):
    """cmx_intra_gram_prefetch_dev -> [another op] -> cmx_intra_compact_range_dev: the records must be those of the vectors
    and weights current at the compact call, i.e. what the same context computes without kept blocks right afterwards"""
    import torch
    I, eng = c.I, c.eng
    n, kind = I.n[sz], engine.STAT_CORRELATION
    npairs = n * (n - 1) // 2
    d_norm, d_ns, d_nm = _dev(I.m["norm"][:n]), _dev(I.null["stat"]), _dev(I.null["nmin"])
    restore = False

    def compact(d_counts):
        out = torch.zeros(npairs * engine.PAIR_COMPACT.itemsize, dtype=torch.uint8, device="cuda")
        eng.intra_compact_range_dev(kind, d_counts, d_norm, d_ns, d_nm, NCLS, out)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(engine.PAIR_COMPACT)

    if between == "map_dev":
        # the vectors come from a device mapping; another alignment is then mapped into the same tensor
        d_counts = torch.zeros(eng.B * eng.K, n, dtype=torch.float64, device="cuda")
        eng.map_sites_dev(_dev(I.aln[:, :n]), counts=d_counts)
        eng.intra_gram_prefetch_dev(kind, d_counts, n)
        eng.map_sites_dev(_dev(I.aln2[:, :n]), counts=d_counts)
    else:
        d_counts = _dev(I.counts[:n].reshape(n, -1).T)
        eng.intra_gram_prefetch_dev(kind, d_counts, n)
        if between == "pair_stats":
            eng.pair_stats(kind, I.counts2[:I.n2[sz]])
        elif between == "set_weights":
            eng.set_statistic_weights(I.w["a" if c.settings.weights == "b" else "b"])
            restore = True
    try:
        rec = compact(d_counts)
        again = compact(d_counts)          # the kept blocks were consumed: this one computes its own
    finally:
        if restore:
            eng.set_statistic_weights(c.weights())
    for f in engine.PAIR_COMPACT.names:
        assert np.array_equal(rec[f], again[f], equal_nan=True), \
            "records made from kept Gram blocks differ from the records computed at the compact call (%s)" % f
    return {f: np.ascontiguousarray(rec[f]) for f in engine.PAIR_COMPACT.names}


def op_group_stats(c, sz):
    return dict(stat=c.eng.group_stats(0, c.I.counts[:c.I.n[sz]], c.I.groups[sz]))


def op_candidate_groups(c, sz):
    win, ok, obs, args = c.I.cand[sz]
    g = c.eng.candidate_groups(0, win, ok, obs, **args)
    return dict(n1=g["n1"], n2=g["n2"], counters=np.array([g["trials"], g["batches"]]))


def op_cluster_sites(c, sz):
    return c.eng.cluster_sites(oc.DIST_CORRELATION, oc.LINK_COMPLETE, c.I.counts[:c.I.n[sz]])


def op_cluster_null(c, sz):
    r0, r1, ns = c.I.cluster_null[sz]
    return c.eng.cluster_null(oc.DIST_CORRELATION, oc.LINK_COMPLETE, 123, r0, r1, ns)


def op_hclust(c, sz):
    return c.eng.hclust(c.I.dist[sz], oc.LINK_AVERAGE)


def _mica_alns(I, sz, unknowns):
    n1, n2 = I.mica_n[sz]
    a1, a2 = (I.mica1u, I.mica2u) if unknowns else (I.mica1, I.mica2)
    return np.ascontiguousarray(a1[:, :n1]), np.ascontiguousarray(a2[:, :n2]), (I.mica_masks if unknowns else None)


def op_mi_columns(c, sz, unknowns=False):
    a1, a2, mk = _mica_alns(c.I, sz, unknowns)
    return c.eng.mi_columns(a1, a2, c.I.A, mk)


def op_mi_pairs(c, sz, unknowns=False):
    a1, a2, mk = _mica_alns(c.I, sz, unknowns)
    i1, i2 = c.I.mica_idx[sz]
    return c.eng.mi_pairs(a1, i1, i2, a2, c.I.A, mk)


def op_perm(c, sz, Ts):
    out = {}
    for k, Tp in enumerate(Ts):
        pv, npm = c.eng.mica_permutation_test(c.I.perm[Tp], 200, 41, nalpha=c.I.A)
        out["pvalue%d" % k], out["nperm%d" % k] = pv, npm
    return out


def op_mica_parametric_null(c, sz):
    nrep, ram = c.I.nrep[sz]
    return c.eng.mica_parametric_null(77, nrep, ram, with_norms=True)


def op_mica_zscore_null(c, sz):
    n = c.I.mica_n[sz][0]
    ns, nk = c.eng.mica_zscore_null(engine.MICA_MIP, c.I.mica_o["mi"][:n, :n].copy(), c.I.mica_o["h1"][:n])
    return dict(stat=ns, key=nk)


def op_mica_average_mi(c, sz):
    n = c.I.mica_n[sz][0]
    avg, full = c.eng.mica_average_mi(c.I.mica_o["mi"][:n, :n].copy())
    return dict(avg=avg, full=np.array([full]))


def _bind(f, **kw):
    return lambda c, sz: f(c, sz, **kw)


CATALOGUE = {
    "map": op_map, "map_masks": _bind(op_map, masks=True), "map_dev": _bind(op_map, dev=True), "map_masks_refused": op_map_masks_refused,
    "asr": op_asr, "asr_masks": _bind(op_asr, masks=True),
    "simulate": op_simulate, "simulate_continuous": op_simulate_continuous,
    "pair_k0": _bind(op_pair, kind=0), "pair_k1": _bind(op_pair, kind=1), "pair_k3": _bind(op_pair, kind=3), "pair_k4": _bind(op_pair, kind=4),
    "pair_k5": _bind(op_pair, kind=5), "pair_k6": _bind(op_pair, kind=6), "pair_k7": _bind(op_pair, kind=7), "pair_k9": _bind(op_pair, kind=9),
    "pair_bounds": _bind(op_pair, kind=8), "pair_k6_slots": op_pair_k6_slots,
    "null_fused": _bind(op_null, which="fused"), "null_supplied": _bind(op_null, which="supplied"),
    "null_continuous": _bind(op_null, which="continuous"), "null_k6": _bind(op_null, which="k6"),
    "null_bounds": _bind(op_null, which="bounds"), "null_inter": _bind(op_null, which="inter"),
    "null_fused_patterns_on": _bind(op_null_fused_patterns, on=True), "null_fused_patterns_off": _bind(op_null_fused_patterns, on=False),
    "null_fused_patterns_auto": _bind(op_null_fused_patterns, on=None),
    "pvalues": op_pvalues, "rows": op_rows, "inter_rows": op_inter_rows,
    "compact_prefetched": _bind(op_compact, between=None), "compact_after_pair_stats": _bind(op_compact, between="pair_stats"),
    "compact_after_set_weights": _bind(op_compact, between="set_weights"), "compact_after_map_dev": _bind(op_compact, between="map_dev"),
    "group_stats": op_group_stats, "candidate_groups": op_candidate_groups, "cluster_sites": op_cluster_sites,
    "cluster_null": op_cluster_null, "hclust": op_hclust,
    "mi_columns": op_mi_columns, "mi_columns_unknowns": _bind(op_mi_columns, unknowns=True),
    "mi_pairs": op_mi_pairs, "mi_pairs_unknowns": _bind(op_mi_pairs, unknowns=True),
    "perm_T30": _bind(op_perm, Ts=(30,)), "perm_T64": _bind(op_perm, Ts=(64,)), "perm_T30_T64_T30": _bind(op_perm, Ts=(30, 64, 30)),
    "mica_parametric_null": op_mica_parametric_null, "mica_zscore_null": op_mica_zscore_null, "mica_average_mi": op_mica_average_mi,
}


def run_op(c, name):
    base, sz = _split(name)
    out = {k: np.asarray(v) for k, v in CATALOGUE[base](c, sz).items() if v is not None}
    assert out and all(v.dtype.kind in "fiub" for v in out.values()), "op %s returned something that cannot be compared" % name
    return out


# ------------------------------------------------------------------------------------------------ the oracle anchors
def _check_map(I, r, o):
    tight = I.name == "c61"                                 # (test_gpu_codon_alphabets.py: the plain kernels, 1e-9 / 1e-12)
    rel_close(r["counts"], o["counts"], 1e-9 if tight else 1e-6, 1e-300)
    rel_close(r["logL"], o["logL"], 1e-12 if tight else 1e-9)
    rel_close(r["post_rate"], o["post_rate"], 1e-12 if tight else 1e-9)
    rel_close(r["norm"], o["norm"], 1e-9 if tight else 1e-6)
    assert np.array_equal(r["rate_class"], o["rate_class"])


def _check_null(r, o):
    rel_close(r["stat"], o["stat"], 1e-6, 1e-12)
    rel_close(r["prmin"], o["prmin"], 1e-9)
    rel_close(r["nmin"], o["nmin"], 1e-6)
    assert np.array_equal(r["rcmin"], o["rcmin"])


def _oracle_pair(I, kind, c1, c2=None):
    if kind == 9:                                           # the raw Gram of the type-0 counts (test_analysis_tools_vector_matrices)
        return c1[:, :, 0] @ (c1 if c2 is None else c2)[:, :, 0].T
    ok, params = kind, None
    if kind == 5:
        params = oracle.stat_params(5, 0.05)
    elif kind == 6:
        params = np.concatenate([I.mv[0], I.mv[0] if c2 is None else I.mv[1]])
    elif kind == 8:
        ok, params = oracle.ST_DISCRETE_MI, np.concatenate([[float(len(BOUNDS))], BOUNDS])
    return oracle.pair_stats_intra(ok, c1, params) if c2 is None else oracle.pair_stats_inter(ok, c1, c2, params)


def anchor(I, name, r):
    """the fresh result of an op at the default settings against the oracle call of its entry point, at the tolerance of
    that entry point's existing parity test"""
    base, sz = _split(name)
    key = ("anchor", name)
    n, n2 = (I.n[sz], I.n2[sz]) if sz else (0, 0)
    if base in ("map", "map_dev", "map_masks", "map_masks_refused"):
        aln = I.aln[:, :5] if base == "map_masks_refused" else (I.aln_amb if base == "map_masks" else I.aln)[:, :I.nmap[sz]]
        _check_map(I, r, oracle.map_sites(I.om, aln, I.masks if base == "map_masks" else None))
    elif base in ("asr", "asr_masks"):
        aln = (I.aln_amb if base == "asr_masks" else I.aln)[:, :I.nmap[sz]]
        o = oracle.map_sites_marginal(I.om, aln, True, masks=I.masks if base == "asr_masks" else None, want_post=True)
        nodes = [k for k in range(len(I.case["parent"])) if (np.asarray(I.case["parent"]) == k).any()]
        post = o["post"][:, nodes].sum(axis=2).transpose(1, 0, 2)
        assert np.max(np.abs(r["post"] - post)) <= 1e-9
        clear = o["margin"][:, nodes].T > 1e-9
        assert np.array_equal(r["states"][clear], o["anc"][:, nodes].T[clear])
        assert np.array_equal(r["states"], r["states_alone"])
    elif base == "simulate":
        aln, cls = oracle.simulate(I.om, 43, 17, r["aln"].shape[1])
        assert np.array_equal(r["aln"], aln) and np.array_equal(r["cls"], cls)
    elif base == "simulate_continuous":
        aln, rates = oracle.simulate_continuous(I.om, 44, 5, r["aln"].shape[1], 0.7, 0.1)
        assert (r["aln"] != aln).mean() < 1e-4      # identical but for draws within an ulp of a boundary of the cumulative row
        rel_close(r["rates"], rates, 1e-12, 1e-300)
    elif base.startswith("pair_k") and base != "pair_k6_slots" or base == "pair_bounds":
        kind = 8 if base == "pair_bounds" else int(base[6:])
        tol = (1e-9, 1e-12) if kind == 8 else (1e-9, 1e-300) if kind == 9 else (1e-6, 1e-12)
        tri = np.triu_indices(n, 1) if kind == 9 else np.indices((n, n)).reshape(2, -1)     # kind 9: i < j, as its parity test
        rel_close(r["intra"][tuple(tri)], _oracle_pair(I, kind, I.counts[:n])[tuple(tri)], *tol)
        rel_close(r["inter"], _oracle_pair(I, kind, I.counts[:n], I.counts2[:n2]), *tol)
    elif base == "pair_k6_slots":
        for i in range(11):
            rel_close(r["mv%d" % i], oracle.pair_stats_intra(6, I.counts[:20], np.concatenate([I.mv[i], I.mv[i]])), 1e-6, 1e-12)
    elif base.startswith("null_"):
        nrep, ram = I.nrep[sz]
        if base == "null_fused" or base.startswith("null_fused_patterns"):
            o = oracle.null_intra(I.om, 0, 777, 0, nrep, ram)
            if base == "null_fused_patterns_on":     # the distinct columns of the simulated alignments, counted on the host
                cols = np.concatenate([oracle.simulate(I.om, 777, (rep * 2 + h) * ram, ram)[0] for rep in range(nrep) for h in range(2)], axis=1)
                assert int(r["mapped"][0]) == np.unique(cols, axis=1).shape[1]
        elif base == "null_supplied":
            o = oracle.null_intra(I.om, 1, 0, 0, nrep, ram, supplied=I.sup[sz])
        elif base == "null_continuous":
            aln, _ = oracle.simulate_continuous(I.om, 31, 0, nrep * 2 * ram, 0.7, 0.1)
            sup = np.ascontiguousarray(aln.reshape(I.T, nrep, 2, ram).transpose(1, 2, 0, 3))
            o = oracle.null_intra(I.om, 0, 31, 0, nrep, ram, supplied=sup)
        elif base == "null_k6":
            o = oracle.null_intra(I.om, 6, 13, 0, nrep, ram, params=np.concatenate([I.mv[2], I.mv[2]]))
        elif base == "null_bounds":
            o = oracle.null_intra(I.om, oracle.ST_DISCRETE_MI, 15, 0, nrep, ram, params=np.concatenate([[float(len(BOUNDS))], BOUNDS]))
        else:
            o = oracle.null_inter(I.om, I.om2, 0, 4242, 1, 1 + nrep, ram)
        _check_null(r, o)
    elif base == "pvalues":
        po, no = oracle.intra_pvalues(I.stat[:n, :n].copy(), I.m["norm"][:n], NCLS, I.null["stat"], I.null["nmin"])
        assert np.array_equal(r["nsim"], no) and np.array_equal(r["pvalue"], po, equal_nan=True)
    elif base == "compact_after_set_weights":      # at the default settings the op sets the weights "b" before its compact call
        ok, worst = wr.close(r["stat"], wr.matrix_gram(0, I.counts[:n], wr.normalise(I.w["b"]))[np.triu_indices(n, 1)], 1e-11, 1e-13)
        assert ok, worst                            # (test_gpu_weighted_statistics.py: RTOL, ATOL)
    elif base in ("rows", "compact_prefetched", "compact_after_pair_stats"):
        _, no = oracle.intra_pvalues(I.stat[:n, :n].copy(), I.m["norm"][:n], NCLS, I.null["stat"], I.null["nmin"])
        iu = np.triu_indices(n, 1)
        if base == "rows":
            assert int(r["all_count"][0]) == len(r["all_i"]) == int(r["few_count"][0]) <= len(iu[0])
            assert int(r["filtered_count"][0]) == len(r["filtered_i"]) <= int(r["all_count"][0])
            order = r["all_i"].astype(np.int64) * n + r["all_j"]
            assert np.all(np.diff(order) > 0) and np.all(r["all_i"] < r["all_j"])           # the reference's (i, j) order
            rel_close(r["all_stat"], I.stat[r["all_i"], r["all_j"]], 1e-6, 1e-12)
            assert np.array_equal(r["all_nsim"], no[r["all_i"], r["all_j"]])
            rel_close(r["filtered_stat"], I.stat[r["filtered_i"], r["filtered_j"]], 1e-6, 1e-12)
            assert np.array_equal(r["filtered_nsim"], no[r["filtered_i"], r["filtered_j"]])
            assert len(r["few_i"]) == min(10, len(iu[0]) - 1, int(r["few_count"][0]))
        else:
            rel_close(r["stat"], I.stat[:n, :n][iu], 1e-6, 1e-12)
            assert np.array_equal(r["nsim"], no[iu].astype(np.uint32))
    elif base == "compact_after_map_dev":
        c2 = oracle.map_sites(I.om, I.aln2[:, :n])["counts"]
        rel_close(r["stat"], oracle.pair_stats_intra(0, c2)[np.triu_indices(n, 1)], 1e-6, 1e-12)
    elif base == "inter_rows":
        so = oracle.pair_stats_inter(0, I.counts[:n], I.m2["counts"][:n2])
        assert int(r["all_count"][0]) == len(r["all_i"]) <= n * n2 and int(r["filtered_count"][0]) == len(r["filtered_i"])
        rel_close(r["all_stat"], so[r["all_i"], r["all_j"]], 1e-6, 1e-12)
        rel_close(r["filtered_stat"], so[r["filtered_i"], r["filtered_j"]], 1e-6, 1e-12)
    elif base == "group_stats":
        exp = np.array([ocand.group_stat(0, [I.counts[i] for i in g], oracle.stat_params(0)) for g in I.groups[sz]])
        rel_close(r["stat"], exp, 1e-6, 1e-12)
    elif base == "candidate_groups":
        win, ok, obs, args = I.cand[sz]
        o = ocand.candidate_groups(I.om, 0, win, ok, obs, **args)
        assert np.array_equal(r["n2"], o["n2"]) and list(r["counters"]) == [o["trials"], o["batches"]]
        assert np.all(np.abs(r["n1"].astype(np.int64) - o["n1"]) <= o["near_ties"])
    elif base == "cluster_sites":
        d = oc.distance_matrix(oc.DIST_CORRELATION, I.counts[:n])
        assert np.allclose(r["dist"], d, rtol=1e-6, atol=1e-12)
        merge, dmax, size = oc.hclust(r["dist"], oc.LINK_COMPLETE)
        assert np.array_equal(r["merge"], merge) and np.array_equal(r["dmax"], dmax) and np.array_equal(r["size"], size)
        stat, nmin = oc.group_properties(oc.DIST_CORRELATION, merge, dmax, I.counts[:n])
        assert np.allclose(r["stat"], stat, rtol=1e-6, atol=1e-9) and np.allclose(r["nmin"], nmin, rtol=1e-6, atol=0)
    elif base == "cluster_null":
        r0, r1, ns = I.cluster_null[sz]
        o = oc.cluster_null(I.om, oc.DIST_CORRELATION, oc.LINK_COMPLETE, 123, r0, r1, ns)
        for k in range(r1 - r0):
            if np.unique(oracle.simulate(I.om, 123, (r0 + k) * ns, ns)[0], axis=1).shape[1] != ns:
                continue        # duplicate columns: distances tie to rounding and the tree is not a function of the data
            assert np.array_equal(r["merge"][k], o[k]["merge"]) and np.array_equal(r["size"][k], o[k]["size"])
            assert np.allclose(r["dmax"][k], o[k]["dmax"], rtol=1e-6, atol=1e-12)
            assert np.allclose(r["stat"][k], o[k]["stat"], rtol=1e-6, atol=1e-9)
            assert np.allclose(r["nmin"][k], o[k]["nmin"], rtol=1e-6, atol=0)
    elif base == "hclust":
        merge, dmax, size = oc.hclust(I.dist[sz], oc.LINK_AVERAGE)
        assert np.array_equal(r["merge"], merge) and np.array_equal(r["dmax"], dmax) and np.array_equal(r["size"], size)
    elif base in ("mi_columns", "mi_columns_unknowns", "mi_pairs", "mi_pairs_unknowns"):
        unknowns = base.endswith("unknowns")
        if key not in I._oracle:
            a1, a2, mk = _mica_alns(I, sz, unknowns)
            I._oracle[key] = oracle.mi_columns(a1, a2, I.A, mk)
        o = I._oracle[key]
        if base.startswith("mi_columns"):
            rel_close(r["mi"], o["mi"], 1e-6, 1e-12)
            rel_close(r["hjoint"], o["hjoint"], 1e-6, 1e-12)
            rel_close(r["h1"], o["h1"], 1e-9, 1e-12)
            rel_close(r["h2"], o["h2"], 1e-9, 1e-12)
        else:
            i1, i2 = I.mica_idx[sz]
            rel_close(r["mi"], o["mi"][i1, i2], 1e-6, 1e-12)
            rel_close(r["hjoint"], o["hjoint"][i1, i2], 1e-6, 1e-12)
    elif base.startswith("perm_"):
        for k, Tp in enumerate({"perm_T30": (30,), "perm_T64": (64,), "perm_T30_T64_T30": (30, 64, 30)}[base]):
            po, no = oracle.mica_permutation_test(I.perm[Tp], I.A, 200, 41)
            assert np.array_equal(r["nperm%d" % k], no) and np.array_equal(r["pvalue%d" % k], po)
    elif base == "mica_parametric_null":
        nrep, ram = I.nrep[sz]
        for rep in range(nrep):
            a1, _ = oracle.simulate(I.om, 77, (rep * 2) * ram, ram)
            a2, _ = oracle.simulate(I.om, 77, (rep * 2 + 1) * ram, ram)
            o = oracle.mi_columns(a1, a2, I.A)
            sl = slice(rep * ram, (rep + 1) * ram)
            rel_close(r["mi"][sl], np.diag(o["mi"]), 1e-6, 1e-12)
            rel_close(r["hjoint"][sl], np.diag(o["hjoint"]), 1e-6, 1e-12)
            rel_close(r["nmin"][sl], np.minimum(oracle.map_sites(I.om, a1)["norm"], oracle.map_sites(I.om, a2)["norm"]), 1e-6, 1e-12)
    elif base == "mica_zscore_null":
        m = I.mica_n[sz][0]
        os_, ok = oracle.mica_zscore_null(1, I.mica_o["mi"][:m, :m], I.mica_o["h1"][:m])
        fin = np.isfinite(os_)
        rel_close(r["stat"][fin], os_[fin], 1e-6, 1e-12)
        rel_close(r["key"], ok, 1e-6, 0.0)
    elif base == "mica_average_mi":
        m = I.mica_n[sz][0]
        avg, full = oracle.mica_average_mi(I.mica_o["mi"][:m, :m])
        rel_close(r["avg"], avg, 1e-6, 1e-12)
        assert abs(r["full"][0] - full) <= 1e-6 * abs(full)
    else:
        raise AssertionError("no oracle anchor for op " + name)


# ------------------------------------------------------------------------------------------------ running and checking
def same(a, b):
    """None if the two results are equal byte for byte (NaN equal to NaN), else the first key that differs"""
    if sorted(a) != sorted(b):
        return "keys"
    for k in sorted(a):
        if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"):
            return k
    return None


class World:
    """the inputs of the three models, the memoised fresh references and the three long-lived contexts"""

    def __init__(self):
        self.inputs = {name: Inputs(name) for name in plan.CONTEXTS}
        self.refs = {}
        self.contexts_made = 0
        self.long = None

    def long_lived(self):
        if self.long is None:
            self.long = {name: Ctx(self.inputs[name]) for name in plan.CONTEXTS}
        return self.long

    def fresh(self, name, op, settings):
        c = Ctx(self.inputs[name])
        self.contexts_made += 1
        try:
            plan.apply_settings(c.eng, settings, c.I.w)
            c.settings = settings.copy()
            return run_op(c, op)
        finally:
            c.close()

    def reference(self, name, op, settings):
        key = (name, op, settings.key())
        if key not in self.refs:
            self.refs[key] = self.fresh(name, op, settings)
        return self.refs[key]

    def check(self, name, op, got, settings, where):
        if op in NOT_BYTE_REPRODUCIBLE:
            try:
                anchor(self.inputs[name], op, got)
            except AssertionError as e:
                raise AssertionError("%s: op %s against the oracle: %s" % (where(), op, e)) from None
            return
        bad = same(got, self.reference(name, op, settings))
        assert bad is None, "%s: output '%s' of op %s differs from the same call on a fresh context" % (where(), bad, op)


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    if w.long is not None:
        for c in w.long.values():
            c.close()


def _where(step, name, op, settings, trail):
    return lambda: "step %d on context %s, op %s, %r, after %s" % (step, name, op, settings, " -> ".join(trail[-5:]) or "nothing")


def run_history(world, contexts, history, reset=True):
    """a [(context, op)] sequence on long-lived contexts; every data step is checked"""
    trail = {name: [] for name in plan.CONTEXTS}
    if reset:   # the contexts come from earlier tests in whatever state those left: only the settings are put back
        for name, c in contexts.items():
            for op in plan.Settings().values():
                c.set(op)
    for step, (name, op) in enumerate(history):
        c = contexts[name]
        if op in plan.SETTING_OPS:
            c.set(op)
        else:
            got = run_op(c, op)
            world.check(name, op, got, c.settings, _where(step, name, op, c.settings, trail[name]))
        trail[name].append(op)


def test_the_catalogue_has_a_closure_for_every_planned_op():
    assert {_split(op)[0] for op in plan.ALL_OP_NAMES} == set(CATALOGUE)


@pytest.mark.parametrize("name", plan.CONTEXTS)
def test_every_op_is_reproducible_on_fresh_contexts_and_matches_the_oracle(world, name):
    """two fresh contexts give the same bytes (all ops but NOT_BYTE_REPRODUCIBLE, see the module docstring), and the
    fresh result -- the reference of every later step -- is what the oracle computes"""
    t0 = time.time()
    default = plan.Settings()
    failures = []
    for op in plan.DATA_OPS[name]:
        try:
            first = world.reference(name, op, default)
            second = world.fresh(name, op, default)
            anchor(world.inputs[name], op, first)
            if op in NOT_BYTE_REPRODUCIBLE:
                anchor(world.inputs[name], op, second)
            else:
                bad = same(first, second)
                assert bad is None, "output '%s' differs between two fresh contexts" % bad
        except (AssertionError, engine.CmxError) as e:
            failures.append("op %s on a fresh %s context: %s: %s" % (op, name, type(e).__name__, str(e)[:300]))
    assert not failures, "\n".join(failures)
    print("%s: %d ops, %.1f s" % (name, len(plan.DATA_OPS[name]), time.time() - t0))


@pytest.mark.parametrize("name", plan.CONTEXTS)
def test_every_ordered_pair_of_ops_on_one_context(world, name):
    """Eulerian circuit of the complete directed graph (loops included) over the context's ops: every (a, b) is a pair
    of neighbours once.  masks -> unfused null -> no masks -> masks, large -> small -> large and the permutation test's
    T = 30 / 64 / 30 are all in it."""
    t0 = time.time()
    walk = plan.pair_walk(name)
    run_history(world, world.long_lived(), [(name, op) for op in walk])
    print("%s: %d steps, %.1f s, %d fresh contexts so far" % (name, len(walk), time.time() - t0, world.contexts_made))


@pytest.mark.parametrize("seed", plan.SEEDS)
def test_random_histories_over_three_contexts_with_settings(world, seed):
    t0 = time.time()
    history = plan.random_history(seed)
    run_history(world, world.long_lived(), history)
    print("seed %d: %d steps, %.1f s, %d fresh contexts so far" % (seed, len(history), time.time() - t0, world.contexts_made))


@pytest.fixture
def guard_on():
    was = engine.scratch_guard(True)
    engine.scratch_guard_failures(clear=True)
    yield
    engine.scratch_shrink(None, 0)
    engine.scratch_guard(was)
    engine.scratch_guard_failures(clear=True)


@pytest.mark.parametrize("name", plan.CONTEXTS)
def test_a_random_history_under_the_scratch_guard(world, guard_on, name):
    """the same history (one alphabet's share of it) on a context created with CMX_SCRATCH_GUARD on: every buffer handed
    out at a smaller logical size than it has grown to carries its canary right behind the logical end"""
    history = [(n, op) for n, op in plan.random_history(plan.SEEDS[0]) if n == name]
    c = Ctx(world.inputs[name])
    try:
        run_history(world, {name: c}, history, reset=False)
        c.eng.synchronize()
        c.eng.scratch_check()
        if c._eng2 is not None:
            c._eng2.scratch_check()
        assert engine.scratch_guard_failures() == []
    finally:
        c.close()
