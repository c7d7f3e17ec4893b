#!/usr/bin/env python3
"""Every output of the plain-kernel stage (cmx_variants.hip: the mapping variants, the plain alphabet, ancestral states) for
a fixed list of cases, without and with per-site likelihood scaling, as one .npz.  A refactor of the stage must leave every
array equal as bytes:

    COMAP_MI355X_LIB=OLD/libcomap_mi355x.so scripts/dump_plain_stage.py old.npz
    COMAP_MI355X_LIB=NEW/libcomap_mi355x.so scripts/dump_plain_stage.py new.npz      # each in a fresh process
    scripts/dump_plain_stage.py --compare old.npz new.npz

Cases: 4, 20 and 61 states x the four nijt.average / nijt.joint settings, with and without counts; a mask table at 4 and
20 states; non-homogeneous model sets, one of them with two substitution types; an alignment per alphabet that crosses a
pass of the mapping and one that crosses a pass of the ancestral states; ancestral states with and without posterior.
Then the same cases once more with set_likelihood_scaling(True) (keys scaled/...), and one case that actually rescales:
tests/scaled_cases.py's long(20, 300) under the four options and its ancestral states with posterior."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OPTIONS = [(True, True), (False, True), (True, False), (False, False)]


def compare(a, b):
    a, b = np.load(a), np.load(b)
    bad = [k for k in sorted(set(a.files) | set(b.files))
           if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
    print(f"{len(a.files)} arrays, {len(bad)} differing", *bad)
    return 1 if bad else 0


def dump(path):
    import oracle
    import model_sets as ms
    import scaled_cases as sc
    from comap_amd import engine, protein_models as pm, synthetic
    out = {}

    def run(tag, eng, aln, masks=None, options=OPTIONS, asr=True):
        eng.set_likelihood_scaling(bool(prefix))
        for average, joint in options:
            eng.set_mapping_options(average, joint)
            for k, v in eng.map_sites(aln, masks=masks).items():
                out[f"{prefix}{tag}/avg{int(average)}joint{int(joint)}/{k}"] = v
            out[f"{prefix}{tag}/avg{int(average)}joint{int(joint)}/norm_only"] = eng.map_sites(aln, masks=masks, want_counts=False)["norm"]
        if asr:
            r = eng.ancestral_states(aln, masks=masks, want_posterior=True)
            out[f"{prefix}{tag}/asr/states"], out[f"{prefix}{tag}/asr/post"] = r["states"], r["post"]
            out[f"{prefix}{tag}/asr/states_only"] = eng.ancestral_states(aln, masks=masks)["states"]

    def model(S):
        if S in (4, 20):
            return synthetic.protein_model(0.5, 4) if S == 20 else synthetic.dna_model(0.5, 4)
        Q, pi = pm.synthetic_reversible(S, 100 + S)
        rates, probs = pm.gamma_rates(0.5, 4)
        return dict(Q=Q, pi=pi, rates=rates, probs=probs)

    star = (np.array([3, 3, 3, -1], dtype=np.int32), np.array([0.11, 0.23, 0.37, 0.0]), np.arange(3, dtype=np.int32))
    for prefix in ("", "scaled/"):
        for S, option, spp in ((4, (True, False), 524288), (20, (False, True), 104704), (61, (True, True), 32768)):
            m = model(S)
            args = (m["Q"], m["pi"], m["rates"], m["probs"])
            eng = engine.Engine(*synthetic.random_tree(9, 40 + S), *args)
            aln = np.random.default_rng(S).integers(0, S, size=(9, 70)).astype(np.uint8)
            aln[:, :40] = oracle.simulate(oracle.Model(*synthetic.random_tree(9, 40 + S), *args), 7, 0, 40)[0]
            aln[2, ::7] = S
            run(f"S{S}", eng, aln)
            if S != 61:
                masks = oracle.default_masks(S)[:S + 3].copy()
                masks[S + 1] = 0b1010
                aln[4, 1::5] = S + 1
                run(f"S{S}/masks", eng, aln, masks=masks)
            eng = engine.Engine(*star, *args)
            long = oracle.simulate(oracle.Model(*star, *args), 900 + S, 0, 2 * spp + 1)[0]      # ancestral states: 2 GiB a pass
            run(f"S{S}/map_pass", eng, long[:, :spp + 1], options=[option], asr=False)
            run(f"S{S}/asr_pass", eng, long, options=[], asr=True)
        for name, K in (("n4x4", 1), ("p20x4", 2), ("c61x2", 1)):
            c = ms.case(name)
            run(f"set/{name}/K{K}", ms.engine_of(c, Bk=ms.registers(c, K)), ms.alignment(c, ambiguous=True),
                masks=ms.IUPAC if c["S"] == 4 else None)
        if prefix:                              # fp64 underflows here without scaling: the exponents are at work
            rescaling = sc.long(20, 300)
            run("long20x300", rescaling.engine(), rescaling.aln)
    np.savez(path, **out)
    print(f"{len(out)} arrays from {engine.LIB_PATH} -> {path}")


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1] == "--compare" else dump(sys.argv[1]))
