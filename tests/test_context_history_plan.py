"""The sequence generator of tests/test_gpu_context_history.py (tests/context_history_plan.py) on the CPU: the pair walk
is an Eulerian circuit, a seed reproduces its history, the fixed seeds reach every (setting, op) combination, and the
shadow record of the settings replays the setter calls.  Nothing here imports torch or loads the engine library."""
import sys
from collections import Counter

import context_history_plan as plan


def test_importing_the_plan_loads_neither_torch_nor_the_engine():
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import context_history_plan; "
            "assert 'torch' not in sys.modules and 'comap_amd.engine' not in sys.modules")
    import os
    subprocess.check_call([sys.executable, "-c", code % os.path.dirname(os.path.abspath(plan.__file__))])


def test_euler_circuit_visits_every_ordered_pair_once():
    for n in (1, 2, 3, 7, 66, 92):
        seq = plan.euler_circuit(n)
        assert len(seq) == n * n + 1 and seq[0] == seq[-1]
        pairs = Counter(zip(seq, seq[1:]))
        assert len(pairs) == n * n and set(pairs.values()) == {1}
        assert set(pairs) == {(a, b) for a in range(n) for b in range(n)}


def test_pair_walk_covers_the_catalogue_of_every_context():
    for ctx in plan.CONTEXTS:
        ops = plan.DATA_OPS[ctx]
        assert len(set(ops)) == len(ops)
        walk = plan.pair_walk(ctx)
        assert len(walk) == len(ops) ** 2 + 1
        assert Counter(zip(walk, walk[1:])) == Counter({(a, b): 1 for a in ops for b in ops})
    # the sequences the issue of this test names are neighbours somewhere: masks -> null -> no masks -> masks is made of
    # ordered pairs, each of which the walk holds
    for ctx in ("p20", "n4"):
        for op in ("map_masks_l", "null_inter_s", "null_bounds_l", "map_l", "map_dev_s", "perm_T30_T64_T30", "pair_k6_slots",
                   "compact_after_set_weights_l", "compact_after_map_dev_s"):
            assert op in plan.DATA_OPS[ctx]
    assert "map_masks_refused" in plan.DATA_OPS["c61"] and not any(op.startswith(("map_masks_", "asr_masks")) and
                                                                   op != "map_masks_refused" for op in plan.DATA_OPS["c61"])


def test_every_data_op_has_two_sizes_or_is_listed_as_unsized():
    for ctx in plan.CONTEXTS:
        ops = set(plan.DATA_OPS[ctx])
        for op in ops:
            if op.endswith("_s"):
                assert op[:-2] + "_l" in ops
            elif op.endswith("_l"):
                assert op[:-2] + "_s" in ops
            else:
                assert op in ("pair_k6_slots", "perm_T30", "perm_T64", "perm_T30_T64_T30", "map_masks_refused")


def test_a_seed_reproduces_its_history():
    for seed in plan.SEEDS:
        assert plan.random_history(seed) == plan.random_history(seed)
    assert plan.random_history(plan.SEEDS[0]) != plan.random_history(plan.SEEDS[1])
    for seed in plan.SEEDS:      # every op of every context once per round, setting ops mixed in on all three contexts
        h = plan.random_history(seed)
        data = Counter((c, op) for c, op in h if op not in plan.SETTING_OPS)
        assert data == Counter({(c, op): plan.ROUNDS for c in plan.CONTEXTS for op in plan.DATA_OPS[c]})
        assert {c for c, op in h if op in plan.SETTING_OPS} == set(plan.CONTEXTS)


def test_the_fixed_seeds_reach_every_setting_and_op_combination():
    got = plan.coverage([plan.random_history(seed) for seed in plan.SEEDS])
    missing = plan.wanted_coverage() - got
    assert not missing, sorted(missing)[:10]
    assert len(plan.wanted_coverage()) == sum(len(plan.DATA_OPS[c]) for c in plan.CONTEXTS) * len(plan.SETTING_OPS)
    # more than one value of a family changes between two runs of the same op, and not only on whole-round boundaries
    keys = {(c, st.key()) for seed in plan.SEEDS for c, _, st in plan.replay(plan.random_history(seed))}
    assert all(sum(1 for c, _ in keys if c == ctx) > plan.ROUNDS for ctx in plan.CONTEXTS)


def test_fused_nulls_run_under_every_null_patterns_value():
    """set_null_patterns is read on the fused path only (averaged joint mapping, no weights).  The explicit ops force
    that path under each value on every step they run (pair walk included); and the histories' own settings bring
    every fused-eligible null of both contexts with a fused null to patterns on and to patterns off while it is fused."""
    for ctx in ("p20", "n4"):
        walk = set(plan.pair_walk(ctx))
        for v in ("on", "off", "auto"):
            for sz in ("_s", "_l"):
                assert "null_fused_patterns_" + v + sz in walk
    assert not any(op.startswith("null_fused_patterns") for op in plan.DATA_OPS["c61"])      # the plain alphabet has no fused null
    got = plan.fused_null_coverage([plan.random_history(seed) for seed in plan.SEEDS])
    want = {(c, v, op + sz) for c in ("p20", "n4") for v in (True, False) for op in plan.FUSED_ELIGIBLE for sz in ("_s", "_l")}
    assert not want - got, sorted(want - got, key=str)
    assert len(set(plan.ORDER_SEEDS.values())) > 1 and set(plan.ORDER_SEEDS) == set(plan.SEEDS)


class _Recorder:
    def __init__(self):
        self.calls = []

    def set_mapping_options(self, average=True, joint=True):
        self.calls.append(("mapping", (average, joint)))

    def set_statistic_weights(self, w=None):
        self.calls.append(("weights", w))

    def set_null_patterns(self, on=None):
        self.calls.append(("patterns", on))


def test_shadow_settings_replay_the_setter_calls_of_the_sequence():
    vectors = {"a": "vector a", "b": "vector b"}
    for seed in plan.SEEDS:
        live = {c: _Recorder() for c in plan.CONTEXTS}
        shadow = {c: plan.Settings() for c in plan.CONTEXTS}
        for step, (c, op) in enumerate(plan.random_history(seed)):
            if op in plan.SETTING_OPS:
                plan.issue_setting(live[c], op, vectors)
                shadow[c].record(op)
            elif step % 97 == 0:
                # what the sequence has left in the context (the last call of each family; families never set: the
                # engine's defaults) is what the shadow record issues on a fresh engine
                last = {"mapping": (True, True), "weights": None, "patterns": None}
                last.update(dict(live[c].calls))
                fresh = _Recorder()
                plan.apply_settings(fresh, shadow[c], vectors)
                assert dict(fresh.calls) == last and len(fresh.calls) == 3
    s = plan.Settings()
    assert s.is_default() and s.values() == ("set_map_avg_joint", "set_weights_none", "set_patterns_auto")
    s.record("set_map_noavg_marginal")
    s.record("set_weights_b")
    assert s.key() == ((False, False), "b", None) and not s.is_default()
