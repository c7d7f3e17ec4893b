"""The call sequences of tests/test_gpu_context_history.py, as plain Python (no torch, no engine library): which ops
each long-lived context has, the walk that makes every ordered pair of them neighbours, the seeded random histories
with the setting ops mixed in, and the shadow record of a context's settings.  tests/test_context_history_plan.py
checks this module on the CPU.

An op is a name; the closures behind the names live in the GPU module (one per name, asserted there).  Data-bearing
ops come in two sizes: `<base>_s` (a few sites, down to one where the entry point allows it) and `<base>_l` (several
times larger), so a sequence moves large -> small -> large through the grow-only scratch buffers."""
import random

# the three contexts alive at once: 20-state G4 (pattern null on by default), 4-state G4 (class-fused walk, cherry
# tables), a codon-sized plain alphabet (every null unfused, no mask tables)
CONTEXTS = ("p20", "n4", "c61")

# ------------------------------------------------------------------------------------------------ settings
# three families; each setting op sets one value of one family and returns nothing
MAPPING_OPTIONS = {"set_map_avg_joint": (True, True), "set_map_avg_marginal": (True, False),
                   "set_map_noavg_joint": (False, True), "set_map_noavg_marginal": (False, False)}
WEIGHTS = {"set_weights_a": "a", "set_weights_b": "b", "set_weights_none": None}
NULL_PATTERNS = {"set_patterns_auto": None, "set_patterns_on": True, "set_patterns_off": False}
FAMILIES = (("mapping", MAPPING_OPTIONS), ("weights", WEIGHTS), ("patterns", NULL_PATTERNS))
SETTING_OPS = tuple(name for _, fam in FAMILIES for name in fam)


class Settings:
    """shadow record of what the setters have left in a context: (average, joint), weights ('a' / 'b' / None: which of
    the test's two weight vectors), null patterns (None automatic / True / False)"""

    def __init__(self, mapping=(True, True), weights=None, patterns=None):
        self.mapping, self.weights, self.patterns = tuple(mapping), weights, patterns

    def copy(self):
        return Settings(self.mapping, self.weights, self.patterns)

    def key(self):
        return (self.mapping, self.weights, self.patterns)

    def is_default(self):
        return self.key() == Settings().key()

    def record(self, op):
        """the setting op `op` has been issued"""
        if op in MAPPING_OPTIONS:
            self.mapping = MAPPING_OPTIONS[op]
        elif op in WEIGHTS:
            self.weights = WEIGHTS[op]
        elif op in NULL_PATTERNS:
            self.patterns = NULL_PATTERNS[op]
        else:
            raise KeyError(op)

    def values(self):
        """the three setting-op names whose values are current"""
        out = []
        for attr, (_, fam) in zip((self.mapping, self.weights, self.patterns), FAMILIES):
            out += [name for name, v in fam.items() if v == attr]
        return tuple(out)

    def __repr__(self):
        return "Settings(average=%s, joint=%s, weights=%r, null_patterns=%r)" % (self.mapping + (self.weights, self.patterns))


def issue_setting(engine, op, weight_vectors):
    """one setting op on an engine (or a recording stub with the same three setters)"""
    if op in MAPPING_OPTIONS:
        engine.set_mapping_options(*MAPPING_OPTIONS[op])
    elif op in WEIGHTS:
        engine.set_statistic_weights(None if WEIGHTS[op] is None else weight_vectors[WEIGHTS[op]])
    elif op in NULL_PATTERNS:
        engine.set_null_patterns(NULL_PATTERNS[op])
    else:
        raise KeyError(op)


def apply_settings(engine, settings, weight_vectors):
    """bring a fresh engine to `settings`: the same setter calls, one per family, as the ops that led there"""
    for op in settings.values():
        issue_setting(engine, op, weight_vectors)


# ------------------------------------------------------------------------------------------------ the catalogue's names
_SIZED = [
    # mapping
    "map", "map_dev", "asr",
    # simulators
    "simulate", "simulate_continuous",
    # pair statistics, intra and inter: kinds 0, 1, 3, 4, 5 (threshold), 6 (mean vectors), 7, 9 and the bounds MI
    "pair_k0", "pair_k1", "pair_k3", "pair_k4", "pair_k5", "pair_k6", "pair_k7", "pair_k9", "pair_bounds",
    # nulls
    "null_fused", "null_supplied", "null_continuous", "null_k6", "null_bounds", "null_inter",
    # p-values and rows
    "pvalues", "rows", "inter_rows",
    "compact_prefetched", "compact_after_pair_stats", "compact_after_set_weights", "compact_after_map_dev",
    # groups and clustering
    "group_stats", "candidate_groups", "cluster_sites", "cluster_null", "hclust",
]
_MASKED = ["map_masks", "asr_masks"]                      # 4 / 20 states only
# the fused null under each value of cmx_set_null_patterns, whatever the context's settings are: the op sets the averaged
# joint mapping, no weights and its pattern value, runs the null and puts the shadow settings back (4 / 20 states: the
# plain alphabet has no fused null)
_FUSED = ["null_fused_patterns_on", "null_fused_patterns_off", "null_fused_patterns_auto"]
# nulls that take the fused path when the mapping is (average, joint) = (yes, yes) and no weights are set
FUSED_ELIGIBLE = ("null_fused", "null_supplied", "null_continuous", "null_k6")
_MICA = ["mi_columns", "mi_columns_unknowns", "mi_pairs", "mi_pairs_unknowns", "mica_parametric_null", "mica_zscore_null",
         "mica_average_mi"]                                                 # alphabets of 4 / 20 letters only
_UNSIZED_ALL = ["pair_k6_slots"]                                            # kind 6 eleven times, eleven mean vectors: the 8 slots wrap
_UNSIZED_MICA = ["perm_T30", "perm_T64", "perm_T30_T64_T30"]                # the cached table's key changes and returns
_PLAIN_ONLY = ["map_masks_refused"]                                         # asserts the refusal, then maps without a table


def _sized(bases):
    return [b + sfx for b in bases for sfx in ("_s", "_l")]


DATA_OPS = {
    "p20": tuple(_sized(_SIZED + _MASKED + _FUSED + _MICA) + _UNSIZED_ALL + _UNSIZED_MICA),
    "n4": tuple(_sized(_SIZED + _MASKED + _FUSED + _MICA) + _UNSIZED_ALL + _UNSIZED_MICA),
    "c61": tuple(_sized(_SIZED) + _UNSIZED_ALL + _PLAIN_ONLY),
}
ALL_OP_NAMES = tuple(sorted({op for ops in DATA_OPS.values() for op in ops}))


# ------------------------------------------------------------------------------------------------ ordered pairs
def euler_circuit(n):
    """vertex sequence of length n * n + 1 over range(n) in which every ordered pair (a, b), loops included, is a pair of
    neighbours exactly once: an Eulerian circuit of the complete directed graph with loops (Hierholzer)"""
    nxt = [0] * n                      # next unused out-edge of each vertex: v -> nxt[v]
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            out.append(stack.pop())
    out.reverse()
    return out


def pair_walk(ctx):
    """every ordered pair of the context's data ops as neighbours, at the default settings: N * N + 1 op names"""
    ops = DATA_OPS[ctx]
    return [ops[i] for i in euler_circuit(len(ops))]


# ------------------------------------------------------------------------------------------------ random histories
SEEDS = (20241, 7, 1303)
ROUNDS = 4     # = the largest family: a seeded order of each family's values, one value per round, reaches them all
# The order in which a history walks each family's values comes from a seed of its own.  Two orders serve the three
# seeds, so that histories share settings (a memoised fresh reference per (op, settings) serves them) and still differ in
# them.  The two are chosen (tests/test_context_history_plan.py asserts it) so that on both contexts that have a fused null
# the fused-eligible state -- mapping (yes, yes), no weights -- meets null patterns on under one order and off under the
# other: otherwise set_null_patterns would only ever be current while the null runs unfused and never reads it.
ORDER_A, ORDER_B = 36, 22
ORDER_SEEDS = {20241: ORDER_A, 7: ORDER_B, 1303: ORDER_A}


def random_history(seed):
    """[(context, op)]: ROUNDS rounds over all three contexts.  A round first issues, per context, the setting ops that
    move it to that round's values (each family walks a seeded shuffle of its values, so a seed's rounds reach every
    value of every family on every context; ORDER_SEEDS picks the shuffles), then every data op of every context once,
    all interleaved in seeded random order -- the setting ops of a context land at random places among the other contexts' data ops."""
    rng, orng = random.Random(seed), random.Random(ORDER_SEEDS[seed])
    orders = {c: [orng.sample(list(fam), len(fam)) for _, fam in FAMILIES] for c in CONTEXTS}
    out = []
    for r in range(ROUNDS):
        lanes = {}
        for c in CONTEXTS:
            setters = [order[r % len(order)] for order in orders[c]]
            rng.shuffle(setters)
            data = list(DATA_OPS[c])
            rng.shuffle(data)
            # a few of the round's data ops run before all of its setters are in: settings change mid-history
            k = rng.randrange(0, 4)
            lane = data[:k] + setters[:1] + data[k:2 * k] + setters[1:] + data[2 * k:]
            lanes[c] = [(c, op) for op in lane]
        while any(lanes.values()):
            c = rng.choice([c for c in CONTEXTS if lanes[c]])
            out.append(lanes[c].pop(0))
    return out


def replay(history):
    """[(context, op, Settings current when the op runs)] for the data ops of a history"""
    cur = {c: Settings() for c in CONTEXTS}
    out = []
    for c, op in history:
        if op in SETTING_OPS:
            cur[c].record(op)
        else:
            out.append((c, op, cur[c].copy()))
    return out


def coverage(histories):
    """{(context, setting op whose value is current, data op)} reached by the histories"""
    got = set()
    for h in histories:
        for c, op, st in replay(h):
            for v in st.values():
                got.add((c, v, op))
    return got


def fused_null_coverage(histories):
    """{(context, null patterns value, op)}: fused-eligible nulls that ran while the mapping was (yes, yes) and no weights
    were set, i.e. on the fused path, where cmx_set_null_patterns is read"""
    return {(c, st.patterns, op) for h in histories for c, op, st in replay(h)
            if st.mapping == (True, True) and st.weights is None and op[:-2] in FUSED_ELIGIBLE}


def wanted_coverage():
    return {(c, v, op) for c in CONTEXTS for op in DATA_OPS[c] for v in SETTING_OPS}
