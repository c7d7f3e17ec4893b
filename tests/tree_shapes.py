"""Catalogue of small tree shapes for the walk and mapping tests (a plain helper module, imported by the tests).

* every unlabelled rooted tree shape with 2..7 leaves, binary and multifurcating (a node may carry all the leaves below it
  as children), each in its canonical child order and, where it differs, mirrored: the walk is sensitive to child order
  (`((0,1),2)` and `(0,(1,2))` are the same shape, but the inlined cherry is the root's first child in one and its second
  in the other);
* the unrooted trees with a trifurcating root that `synthetic.random_tree` makes (3..7 taxa);
* `balanced` / `caterpillar`: rooted binary trees of any size (the cherry-table tests' shapes).

Conventions are the engine's: nodes in post-order (children before parents, root last), `parent[root] = -1`, `blen` with
0 at the root, `leaf_of_taxon[t]` = node id of taxon t.  Leaf labels come from a seeded permutation, so taxon order is not
post-order.  `blen_variants` gives the branch-length variants every shape is run with."""
import itertools
from functools import lru_cache

import numpy as np

from comap_amd import synthetic


# ------------------------------------------------------------------------------------------------ shapes as strings
# a shape is written "x" (leaf) or "(a,b,...)"; canonical = children sorted as strings, so equal shapes are equal strings
def _canon(children):
    return "(" + ",".join(sorted(children)) + ")"


def _partitions(n, k_min=2, largest=None):
    """partitions of n into at least k_min parts, non-increasing"""
    largest = n if largest is None else largest
    if n == 0:
        if k_min <= 0:
            yield ()
        return
    for p in range(min(n, largest), 0, -1):
        for rest in _partitions(n - p, k_min - 1, p):
            yield (p,) + rest


@lru_cache(maxsize=None)
def rooted_shapes(n):
    """every unlabelled rooted shape with n leaves (no node of one child), canonical strings, sorted"""
    if n == 1:
        return ("x",)
    out = set()
    for parts in _partitions(n):
        for pick in itertools.product(*(rooted_shapes(p) for p in parts)):
            out.add(_canon(pick))
    return tuple(sorted(out))


def _parse(s):
    """shape string -> nested lists ("x" -> None)"""
    pos = 0

    def node():
        nonlocal pos
        if s[pos] == "x":
            pos += 1
            return None
        assert s[pos] == "("
        pos += 1
        kids = [node()]
        while s[pos] == ",":
            pos += 1
            kids.append(node())
        assert s[pos] == ")"
        pos += 1
        return kids
    t = node()
    assert pos == len(s)
    return t


def _mirror(t):
    return None if t is None else [_mirror(c) for c in reversed(t)]


def _show(t):
    return "x" if t is None else "(" + ",".join(_show(c) for c in t) + ")"


# ------------------------------------------------------------------------------------------------ arrays
def _arrays(t, seed):
    """nested lists -> (parent, leaf_of_taxon) in post-order; taxa permuted by a seeded permutation"""
    parent = []

    def visit(u):
        kids = [] if u is None else [visit(c) for c in u]
        me = len(parent)
        parent.append(-1)
        for c in kids:
            parent[c] = me
        return me
    visit(t)
    par = np.array(parent, dtype=np.int32)
    is_leaf = np.ones(len(par), dtype=bool)
    is_leaf[par[par >= 0]] = False
    leaves = np.flatnonzero(is_leaf)
    perm = np.random.default_rng(seed).permutation(len(leaves))
    lot = np.zeros(len(leaves), dtype=np.int32)
    lot[perm] = leaves                                   # the i-th leaf in post-order carries taxon perm[i]
    return par, lot


class Shape:
    """one tree topology: name, parent (post-order), leaf_of_taxon, rooted (False: random_tree's trifurcating root)"""

    def __init__(self, name, parent, lot, rooted=True):
        self.name, self.parent, self.lot, self.rooted = name, np.asarray(parent, np.int32), np.asarray(lot, np.int32), rooted
        self.ntaxa, self.nn = len(self.lot), len(self.parent)

    def __repr__(self):
        return f"Shape({self.name})"

    def children(self):
        kids = [[] for _ in range(self.nn)]
        for c, p in enumerate(self.parent):
            if p >= 0:
                kids[p].append(c)
        return kids

    def is_leaf(self):
        leaf = np.zeros(self.nn, dtype=bool)
        leaf[self.lot] = True
        return leaf

    def cherries(self):
        """non-root tree nodes with exactly two children, both leaves: the nodes a class-fused walk inlines"""
        kids, leaf, root = self.children(), self.is_leaf(), self.nn - 1
        return [n for n in range(self.nn) if n != root and len(kids[n]) == 2 and all(leaf[c] for c in kids[n])]

    def internal_nonroot(self):
        leaf = self.is_leaf()
        return [n for n in range(self.nn - 1) if not leaf[n]]

    def blen_variants(self):
        """[(variant name, blen)]: all 0.1; one leaf branch 0; one internal (tree, not pseudo) branch 0 (shapes that have
        one); one saturated branch (5.0); all 1e-6.  The root's entry is 0 in every variant."""
        rng = np.random.default_rng(self.nn * 131 + self.ntaxa)
        base = np.full(self.nn, 0.1)
        base[-1] = 0.0
        out = [("b0.1", base)]
        b = base.copy()
        b[self.lot[int(rng.integers(self.ntaxa))]] = 0.0
        out.append(("leaf0", b))
        inner = self.internal_nonroot()
        if inner:
            b = base.copy()
            b[inner[int(rng.integers(len(inner)))]] = 0.0
            out.append(("inner0", b))
        b = base.copy()
        b[int(rng.integers(self.nn - 1))] = 5.0
        out.append(("sat5", b))
        b = np.full(self.nn, 1e-6)
        b[-1] = 0.0
        out.append(("b1e-6", b))
        return out


def rooted_catalogue(nmin=2, nmax=7):
    """every rooted shape with nmin..nmax leaves, canonical order and (where different) mirrored"""
    out = []
    for n in range(nmin, nmax + 1):
        for s in rooted_shapes(n):
            t = _parse(s)
            for tt in (t, _mirror(t)) if _show(_mirror(t)) != s else (t,):
                name = _show(tt)
                par, lot = _arrays(tt, seed=len(out) + 17 * n)
                out.append(Shape(name, par, lot))
    return out


def unrooted_catalogue(nmin=3, nmax=7, seed=5):
    """random_tree's unrooted binary trees (a trifurcating root), one per size"""
    out = []
    for n in range(nmin, nmax + 1):
        parent, _, lot = synthetic.random_tree(n, seed + n)
        out.append(Shape(f"unrooted{n}", parent, lot, rooted=False))
    return out


def catalogue(nmin=2, nmax=7):
    return rooted_catalogue(nmin, nmax) + unrooted_catalogue(max(nmin, 3), nmax)


def by_name(name, shapes=None):
    for s in shapes if shapes is not None else catalogue():
        if s.name == name:
            return s
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ larger rooted shapes
def _balanced(ntaxa):
    """perfectly balanced rooted binary tree, leaves first (post-order with the root last): every leaf sits in a cherry"""
    nodes, parent = list(range(ntaxa)), {}
    nxt = ntaxa
    level = nodes
    while len(level) > 1:
        up = []
        for k in range(0, len(level) - 1, 2):
            parent[level[k]] = parent[level[k + 1]] = nxt
            up.append(nxt)
            nxt += 1
        if len(level) % 2:
            up.append(level[-1])
        level = up
    nn = nxt
    # renumber in post-order (children before parents, root last)
    kids = {}
    for c, p in parent.items():
        kids.setdefault(p, []).append(c)
    order = []

    def visit(n):
        for c in kids.get(n, []):
            visit(c)
        order.append(n)
    visit(level[0])
    new = {old: i for i, old in enumerate(order)}
    par = np.full(nn, -1, dtype=np.int32)
    for c, p in parent.items():
        par[new[c]] = new[p]
    lot = np.array([new[t] for t in range(ntaxa)], dtype=np.int32)
    return par, lot


def _caterpillar(ntaxa):
    """((((t0, t1), t2), t3) ...): one cherry at the bottom, every other leaf pendant"""
    nn = 2 * ntaxa - 1
    par = np.full(nn, -1, dtype=np.int32)
    lot = np.zeros(ntaxa, dtype=np.int32)
    # post-order: t0, t1, i0, t2, i1, t3, i2, ...
    lot[0], lot[1] = 0, 1
    par[0] = par[1] = 2
    cur = 2
    for t in range(2, ntaxa):
        leaf, inner = cur + 1, cur + 2
        lot[t] = leaf
        par[cur] = par[leaf] = inner
        cur = inner
    return par, lot
