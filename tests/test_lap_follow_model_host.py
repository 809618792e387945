"""tests/lap_follow_model.Follow against tests/lap_view_model: with no priority
updates the leaves a live view has followed to are view_leaves() of the final
rings -- what a fresh lap_view_build computes -- for both call sets of
tests/test_lap_follow_gpu.py, and kept is the count of positive leaves.  Also
pins what those call sets exercise (wraps, idle strata, evicted kept rows), so
the GPU tests keep covering it."""
import numpy as np
import pytest

from lap_follow_model import Follow
from lap_view_model import F, make_calls, view_leaves

SETS = dict(
    small=dict(E=3, C=13, keeps=([0], [1, 3], [0, 1, 2, 3]), calls=(11, 3, 5, 2, 14, 9, [0.6, 0.3, 0.1], 4)),
    large=dict(E=2, C=5000, keeps=([0], [1, 3], [0, 1, 2, 3]), calls=(12, 2, 5, 2, 20, 700, [0.5, 0.5], 4)),
)


def _run(name):
    sh = SETS[name]
    m = Follow(sh["E"], sh["C"], sh["keeps"])
    ready = np.zeros(len(sh["keeps"]), dtype=np.int64)
    for c in make_calls(*sh["calls"]):
        m.add_batch(c["strata"], c["active"], c["source"])
        for k, v in enumerate(m.views):
            # kept is the count of positive leaves, which are the kept sources' filled slots
            for s in range(m.E):
                lv, kept = view_leaves(np.ones(m.C, dtype=F), m.rings.source[s], m.rings.size[s], v.keep, False)
                assert np.array_equal(v.leaves[s], lv), (name, k, s)
                assert v.kept[s] == kept.sum() == (v.leaves[s] > 0).sum()
            ready[k] += v.ready()
    return m, ready


@pytest.mark.parametrize("name", ["small", "large"])
def test_followed_leaves_are_the_view_leaves_of_the_final_rings(name):
    m, _ = _run(name)
    for v in m.views:
        assert v.maxp == 1 and set(np.unique(v.leaves)) <= {F(0), F(1)}
    full = m.views[2]
    assert np.array_equal(full.kept, m.rings.size)  # every source kept: every stored row


def test_what_the_small_call_set_exercises():
    m, ready = _run("small")
    assert m.wraps.tolist() == [3, 1, 0] and m.rings.size.tolist() == [13, 13, 10]
    assert m.idle == 9
    assert [v.lost for v in m.views] == [16, 16, 0]
    assert ready[:2].tolist() == [11, 13]


def test_what_the_large_call_set_exercises():
    m, _ = _run("large")
    assert m.wraps.tolist() == [1, 1]
    assert [v.lost for v in m.views[:2]] == [206, 300]
