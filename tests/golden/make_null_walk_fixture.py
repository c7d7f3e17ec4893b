#!/usr/bin/env python3
"""Known answers on a deeper tree at the edges of branch length and rate, in 50-digit arithmetic (mpmath): the cases
operator_edge_cases.DEEP_CASES on the 12-leaf tree "t12" (tests/operator_edge_cases.py), whose mapping walk stores and loads
workspace vectors and whose cherries have more than the root above them.

Everything is computed by the functions of make_operator_edge_fixture.py (imported, not copied): the spectrum with its two
self-checks of the count integral (plain quotient at 200 digits for every stored time, Gauss-Legendre quadrature at t = 0.3
and 3), pruning down and up, and the averaged joint counts.  The file is not written if a self-check fails.

Stored, rounded to fp64, per case: the inputs, aln [12, 45] (drawn by oracle.simulate under the case's own tree: no site is
impossible, zero-length sisters come out equal; no unknowns), counts [45, 21, K], logL, post_rate, rate_class, class_clear.
No operators and none of the other nijt options.  The file holds data only.

    python tests/golden/make_null_walk_fixture.py        # a few minutes; writes tests/golden/null_walk_edges.npz"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_operator_edge_fixture as mk  # noqa: E402  (puts the repository root and tests/ on the path)

oe = mk.oe


def solve(name):
    i = oe.Inputs(name)
    aln, _ = i.draw()
    assert aln.shape == (len(i.lot), oe.DEEP_NSITES) and (aln < i.S).all(), name
    return mk.solve_case(name, inputs=i, variants=False, store_P=False)


if __name__ == "__main__":
    only = sys.argv[1:]
    out = {}
    for name in oe.DEEP_CASES:
        if only and not any(name.startswith(o) for o in only):
            continue
        t0 = time.time()
        out.update(solve(name))
        print(f"{name} ({time.time() - t0:.0f} s)", flush=True)
    if only:            # a trial run of some cases: nothing is written
        sys.exit(0)
    mk.write_npz(os.path.join(HERE, "null_walk_edges.npz"), out)
