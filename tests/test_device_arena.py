"""The carver behind every staging buffer and device swarm front (include/smooth_feedback_amd/detail/device_arena.hpp):
its layout part is plain C++, checked here through the example harness.  CPU only."""
from examples import models_lib as M


def test_arena_layout_selftest():
    # mixed element types, odd counts, a zero-count entry: total == end of the last array, every pointer aligned to its
    # type, arrays disjoint and in declaration order; one array past the fixed capacity is reported and binds nothing
    assert M.lib().sfbx_arena_selftest() == 0
