"""Hand-built trees for the LDS-slot tests (a plain helper module, imported by the tests).

The mapping walk keeps a short-lived workspace vector in one LDS slot per wave (cmx_walk.h, kLdsSlot).  Candidates exist
only at a node whose two children are both visited nodes -- `(x,(x,x))` is the smallest visited subtree: a leaf beside an
inlined cherry.  Shapes are written as in tree_shapes.py, children in visit order."""
from comap_amd import synthetic
from tree_shapes import Shape, _arrays, _parse

V = "(x,(x,x))"                      # smallest visited subtree
T6 = f"({V},{V})"                    # ((a,(b,c)),(d,(e,f))): smallest tree with a two-visited node, here the root

HAND_BUILT = {
    "root6": T6,
    "nested9": f"({V},{T6})",        # T6 is child B (visited last, handed over) of a second two-visited node: nested intervals
    "disjoint9": f"({T6},{V})",      # T6 is child A: its interval ends before the outer one begins
    # the unrooted forms: one of the root's edges contracted, a trifurcating root (split into a pseudo node on the device)
    "unrooted6": f"({V},x,(x,x))",
    "unrooted9": f"({V},{V},{V})",
    "unrooted9b": f"({T6},x,(x,x))",
}


def hand_built():
    out = []
    for i, (name, s) in enumerate(HAND_BUILT.items()):
        par, lot = _arrays(_parse(s), seed=900 + i)
        out.append(Shape(name, par, lot, rooted=not name.startswith("unrooted")))
    return out


def bench64():
    """the benchmark's 64-taxon tree -> (Shape, blen)"""
    parent, blen, lot = synthetic.random_tree(64, 20260101)
    return Shape("bench64", parent, lot, rooted=False), blen
