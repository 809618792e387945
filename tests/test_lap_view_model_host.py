"""The numpy model the view tests compare the GPU with (tests/lap_view_model.py)
is self-consistent on the host: on masked trees with integer leaves the
descent with the `left > 0` term returns searchsorted_left(cumsum(p), u * sum)
for u > 0 and the first kept slot for u == 0, never a masked slot; on trees
without masked leaves it returns the leaf the rule without the term returns."""
import numpy as np

from lap_view_model import F, build_tree, cap_of, descend, prefix_sum, sample_index, searchsorted_left

US = [0.0, 2.0 ** -24, 1.0 - 2.0 ** -24] + [j / 64 for j in range(1, 64)]


def _cases(seed, n):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        capacity = int(rng.integers(3, 201))
        size = int(rng.integers(1, capacity + 1))
        yield rng, capacity, size


def test_the_tree_model_sums_pairwise():
    T = build_tree([1, 2, 3, 4, 5], 8)
    assert T.dtype == F and T[0] == 0
    assert T[8:16].tolist() == [1, 2, 3, 4, 5, 0, 0, 0]
    assert T[4:8].tolist() == [3, 7, 5, 0] and T[2:4].tolist() == [10, 5] and T[1] == 15
    assert prefix_sum(T, 8, 3) == 6 and prefix_sum(T, 8, 8) == 15 and prefix_sum(T, 8, 0) == 0


def test_masked_trees_never_return_a_masked_slot():
    old_foreign = 0
    for rng, capacity, size in _cases(1, 300):
        cap = cap_of(capacity)
        kept = rng.uniform(0, 1, size) < rng.uniform(0.1, 0.9)
        kept[int(rng.integers(0, size))] = True  # at least one kept row
        prio = rng.integers(1, 6, size).astype(F)
        leaves = np.where(kept, prio, F(0))
        T = build_tree(leaves, cap)
        first = int(np.flatnonzero(kept)[0])
        for u in US:
            i = sample_index(T, cap, size, u)
            assert kept[i], (capacity, size, u, i)
            assert i == (first if u == 0 else searchsorted_left(leaves, u)), (capacity, size, u)
            old_foreign += not kept[sample_index(T, cap, size, u, amended=False)]
    assert old_foreign > 0  # the rule without the term does walk to masked slots (at u == 0)


def test_unmasked_trees_keep_their_leaf():
    for rng, capacity, size in _cases(2, 300):
        cap = cap_of(capacity)
        integer = rng.uniform() < 0.5
        leaves = (rng.integers(1, 6, size) if integer else rng.uniform(0.05, 5.0, size)).astype(F)
        T = build_tree(leaves, cap)
        tot = prefix_sum(T, cap, size)
        for u in US:
            i = sample_index(T, cap, size, u)
            assert i == sample_index(T, cap, size, u, amended=False), (capacity, size, u)
            assert descend(T, cap, F(u) * tot) < size  # the i >= size clamp does not fire
            if integer:
                assert i == searchsorted_left(leaves, u), (capacity, size, u)
