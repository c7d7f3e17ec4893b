"""The case list of tests/cpp/host_model_dump.cpp (a plain helper module, imported by tests/test_host_model_cpp.py and by
scripts/compare_host_model.py): every tree shape the walk tests have, crossed with a model for every layout the host
builds, and a list of inputs that are wrong in two ways, so that the message that wins is pinned.

    write(path) -> (names of the valid cases, names of the error cases)
"""
import numpy as np

import lds_slot_trees
import tree_shapes
from comap_amd import synthetic as sy
from test_traversal_program import _random_multifurcating


# ------------------------------------------------------------------------------------------------ trees
def shapes():
    """[(name, parent, blen, lot, small)]; small: the shapes the two expensive models are crossed with"""
    out = []
    for i, s in enumerate(tree_shapes.catalogue(2, 7)):
        variants = s.blen_variants()
        out.append((f"cat{i}", s.parent, variants[i % len(variants)][1], s.lot, s.ntaxa <= 4))
    for i, s in enumerate(lds_slot_trees.hand_built()):
        blen = np.random.default_rng(40 + i).exponential(0.1, s.nn) + 1e-6
        out.append((s.name, s.parent, blen, s.lot, True))
    s, blen = lds_slot_trees.bench64()
    out.append((s.name, s.parent, blen, s.lot, True))
    n = 20
    out.append(("star20", np.array([n] * n + [-1]), np.full(n + 1, 0.1), np.arange(n), False))
    par, lot = tree_shapes._caterpillar(12)
    out.append(("caterpillar12", par, np.random.default_rng(12).exponential(0.1, len(par)) + 1e-6, lot, False))
    par, blen, lot = _random_multifurcating(30, 7)
    out.append(("multifurcating30", par, blen, lot, False))
    return out


# ------------------------------------------------------------------------------------------------ models
def _reversible(S, seed, base=None):
    """a reversible generator of mean rate 1 with its own frequencies: random exchangeabilities, or those of `base` times
    symmetric random factors -> (Q, pi)"""
    rng = np.random.default_rng(seed)
    if base is None:
        R = rng.uniform(0.2, 2.0, size=(S, S))
    else:
        R = np.asarray(base["Q"]) / np.asarray(base["pi"])[None, :]
    F = rng.uniform(0.5, 1.5, size=(S, S))
    pi = rng.dirichlet(np.full(S, 8.0))
    Q = (R + R.T) / 2 * (F + F.T) / 2 * pi[None, :]
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q / -(pi * np.diag(Q)).sum(), pi


def _two_types(Q, seed):
    W = np.random.default_rng(seed).uniform(-1, 1, size=Q.shape)
    return np.stack([sy.weighted_register(Q, W), sy.weighted_register(Q)])


def _homogeneous(m, **kw):
    S = len(m["pi"])
    d = dict(nstates=S, nclasses=len(m["rates"]), ntypes=1, count_method=0, clamp_negative=1, nmodels=0,
             Q=m["Q"], pi=m["pi"], rates=m["rates"], probs=m["probs"])
    d.update(kw)
    return d


def _model_set(S, C, seed):
    base = sy.protein_model(0.5, C) if S == 20 else sy.dna_model(0.6, C)
    gens = [_reversible(S, seed + g, base) for g in range(2)]
    return dict(nstates=S, nclasses=C, ntypes=1, count_method=0, clamp_negative=1, nmodels=2, rates=base["rates"], probs=base["probs"],
                Qs=np.array([g[0] for g in gens]), pis=np.array([g[1] for g in gens]),
                root_freqs=np.random.default_rng(seed).dirichlet(np.full(S, 5.0)))


def models():
    """[(name, fields, lds_slot, small only)]"""
    p4 = sy.protein_model(0.5, 4)
    out = [("p20x4", _homogeneous(p4), 1, False),
           ("p20x4k2", _homogeneous(p4, ntypes=2, Bk=_two_types(p4["Q"], 1)), 1, True),
           ("p20x4noslot", _homogeneous(p4), 0, False)]
    for C in (3, 4, 5, 8):
        out.append((f"n4x{C}", _homogeneous(sy.dna_model(0.6, C)), 1, False))
    n4 = sy.dna_model(0.6, 4)
    out.append(("n4x4k2", _homogeneous(n4, ntypes=2, Bk=_two_types(n4["Q"], 2)), 1, False))
    for S, C, small in ((7, 2, False), (61, 1, True)):
        Q, pi = _reversible(S, S)
        rates, probs = sy.pm.gamma_rates(0.7, C)
        out.append((f"s{S}x{C}", _homogeneous(dict(Q=Q, pi=pi, rates=rates, probs=probs)), 1, small))
    out.append(("set20x4", _model_set(20, 4, 200), 1, False))
    out.append(("set4x4", _model_set(4, 4, 400), 1, False))
    out.append(("naive20x4", _homogeneous(p4, count_method=1, naive_weights=np.random.default_rng(3).uniform(0.5, 2.0, size=(20, 20))), 1, False))
    out.append(("noclamp4x4k2", _homogeneous(n4, ntypes=2, Bk=_two_types(n4["Q"], 2), clamp_negative=0), 1, False))
    return out


# ------------------------------------------------------------------------------------------------ inputs wrong in two ways
def errors():
    """[(name, tree fields, model fields, mob or None)]; the first named fault is the one the parent's order reports"""
    par, blen, lot = sy.random_tree(6, 11)
    nn = len(par)
    tree = dict(nnodes=nn, ntaxa=6, parent=par, blen=blen, lot=lot)
    p4, n4 = _homogeneous(sy.protein_model(0.5, 4)), _homogeneous(sy.dna_model(0.6, 4))
    out = []
    swapped = par.copy()
    swapped[2] = 1
    out.append(("nstates_vs_postorder", dict(tree, parent=swapped), dict(p4, nstates=65), None))
    out.append(("nclasses_vs_ntypes", tree, dict(p4, nclasses=0, ntypes=65, Bk=_two_types(p4["Q"], 1)), None))
    noQ = dict(p4)
    del noQ["Q"]
    out.append(("Q_vs_incomplete_tree", dict(tree, nnodes=2), noQ, None))
    neg, dup = blen.copy(), lot.copy()
    neg[1] = -0.1
    dup[1] = dup[0]
    out.append(("blen_vs_duplicate_taxon", dict(tree, blen=neg, lot=dup), p4, None))
    # ((t0, t1) u) v with u unary: nodes t0, t1, i, u, t2, root
    unary = dict(nnodes=6, ntaxa=3, parent=np.array([2, 2, 3, 5, 5, -1]), blen=np.full(6, 0.1), lot=np.array([0, 1, 4]))
    out.append(("unary_vs_probs", unary, dict(n4, probs=np.asarray(n4["probs"]) * 0.5), None))
    s4 = _model_set(4, 4, 400)
    noQs = dict(s4, rates=-np.asarray(s4["rates"]))
    del noQs["Qs"]
    out.append(("Qs_vs_rates", tree, noQs, np.arange(nn) % 2))
    irreversible = np.array(s4["Qs"])
    irreversible[0, 0, 1] += 0.2
    irreversible[0, 0, 0] -= 0.2
    mob = np.arange(nn) % 2
    mob[3] = 2
    out.append(("mob_vs_irreversible", tree, dict(s4, Qs=irreversible), mob))
    rows = np.array(s4["Qs"])
    rows[1, 0, 0] += 0.1
    out.append(("row_sum_in_generator_1", tree, dict(s4, Qs=rows), np.arange(nn) % 2))
    return out


# ------------------------------------------------------------------------------------------------ the file
def _fields(kind, name, d):
    parts = [kind, name]
    for k, v in d.items():
        if np.ndim(v) == 0:
            parts += [k, str(int(v))]
        else:
            a = np.asarray(v).ravel()
            vals = [float(x).hex() for x in a] if k not in ("parent", "lot") else [str(int(x)) for x in a]
            parts += [k, str(len(a))] + vals
    return " ".join(parts + ["end"])


def _mob(mob):
    return ["mob", str(len(mob))] + [str(int(x)) for x in mob]


def write(path):
    lines, valid, bad = [], [], []
    ms, ts = models(), shapes()
    for name, d, _, _ in ms:
        lines.append(_fields("model", name, d))
    for name, par, blen, lot, _ in ts:
        lines.append(_fields("tree", name, dict(nnodes=len(par), ntaxa=len(lot), parent=par, blen=blen, lot=lot)))
    for mname, d, slot, small_only in ms:
        for tname, par, _, _, small in ts:
            if small_only and not small:
                continue
            case = ["case", f"{mname}/{tname}", tname, mname, str(slot)]
            if d["nmodels"]:
                case += _mob(np.arange(len(par)) % d["nmodels"])      # generators alternate along the node order
            lines.append(" ".join(case + [";"]))
            valid.append(f"{mname}/{tname}")
    for name, t, m, mob in errors():
        lines.append(_fields("tree", "err_" + name, t))
        lines.append(_fields("model", "err_" + name, m))
        lines.append(" ".join(["case", "error/" + name, "err_" + name, "err_" + name, "1"] + (_mob(mob) if mob is not None else []) + [";"]))
        bad.append("error/" + name)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return valid, bad
