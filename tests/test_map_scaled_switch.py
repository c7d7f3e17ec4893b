"""cmx_debug_map_scaled_plain is host-only process state: exported, declared in the header, off by default, and a set returns the
previous state (no GPU needed).  What it selects is tested in tests/test_gpu_map_scaled_wide.py."""
import os

from comap_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_switch_is_exported_and_declared():
    assert "cmx_debug_map_scaled_plain" in engine.EXPORTS
    assert hasattr(engine.load_library(), "cmx_debug_map_scaled_plain")
    with open(os.path.join(ROOT, "include", "comap_mi355x.h")) as f:
        assert "int cmx_debug_map_scaled_plain(int on);" in f.read()


def test_switch_round_trips_without_a_context():
    was = engine.map_scaled_plain(None)
    try:
        assert was is False
        assert engine.map_scaled_plain(True) is False
        assert engine.map_scaled_plain(None) is True
        assert engine.map_scaled_plain(False) is True
        assert engine.map_scaled_plain(None) is False
    finally:
        engine.map_scaled_plain(was)


def test_the_two_switches_are_independent():
    was = engine.map_scaled_plain(None), engine.map_wide_plain(None)
    try:
        engine.map_scaled_plain(True)
        assert engine.map_wide_plain(None) is False
        engine.map_wide_plain(True)
        engine.map_scaled_plain(False)
        assert engine.map_wide_plain(None) is True
    finally:
        engine.map_scaled_plain(was[0])
        engine.map_wide_plain(was[1])
