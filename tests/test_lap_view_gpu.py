"""LAP.view / LapView (lap_view_build, the descent's `left > 0` term): a view's
trees against the numpy fp32 pairwise tree of tests/lap_view_model.py, its
draws against searchsorted_left, and 50 rounds of sampling and priority updates
that must never reach, or give a priority to, a foreign row.

Small: 3 strata of 37 slots (cap 64), 4 sources, the view keeps {0, 2}.
Large: 3 strata of 5,000 slots (cap 8,192: the build's two leaf blocks and its
second pass, the update kernels' global levels).  In stratum 1 the first and
the last filled slot hold source 3, foreign to the view.  Every comparison is
exact."""
import functools

import numpy as np
import pytest
import torch

from lap_view_model import F, Rings, build_tree, cap_of, make_calls, searchsorted_left, view_leaves

pytestmark = pytest.mark.gpu

E, K, S, A = 3, 4, 80, 7
KEEP = (0, 2)
SHAPES = dict(small=dict(C=37, calls=5, n=24, probs=[0.6, 0.15, 0.25]),
              large=dict(C=5000, calls=3, n=4000, probs=[1 / 3, 1 / 3, 1 / 3]))
ROWS = ("state", "action", "next_state", "reward", "not_done")
ARGS = ("state", "action", "next_state", "reward", "done", "strata", "active")
US = [0.0, 2.0 ** -24, 1.0 - 2.0 ** -24] + [j / 64 for j in range(1, 64)]


@functools.lru_cache(maxsize=None)
def _calls(shape):
    sh = SHAPES[shape]
    calls = make_calls(7, E, S, A, sh["calls"], sh["n"], sh["probs"], K)
    # stratum 1 (never wraps) holds no row of source 1, and its first and its last row come from source 3
    for c in calls:
        c["source"][(c["strata"] == 1) & (c["source"] == 1)] = 3
    first = next((j, i) for j, c in enumerate(calls) for i in range(sh["n"]) if c["active"][i] and c["strata"][i] == 1)
    last = next((j, i) for j, c in reversed(list(enumerate(calls))) for i in reversed(range(sh["n"]))
                if c["active"][i] and c["strata"][i] == 1)
    for j, i in (first, last):
        calls[j]["source"][i] = 3
    return calls


def _base(shape, batch_size=4):
    from exo_amd.replay import LAP
    C = SHAPES[shape]["C"]
    base = LAP(S, A, "cuda", E, max_size=C, batch_size=batch_size)
    model = Rings(E, C)
    for c in _calls(shape):
        t = {k: torch.as_tensor(v, device="cuda") for k, v in c.items()}
        base.add_batch(*[t[k] for k in ARGS], source=t["source"])
        model.add_batch(c["strata"], c["active"], c["source"])
    torch.cuda.synchronize()
    n1 = int(model.size[1])
    assert 1 < n1 < C and model.source[1, 0] == 3 and model.source[1, n1 - 1] == 3
    assert all(np.isin(model.source[s, :model.size[s]], KEEP).any() for s in range(E))
    return base, model


def _update_base(base, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for _ in range(3):
        base.sample()
        base.update_priority(1.0 + 4.0 * torch.rand(E * base.batch_size, device="cuda", generator=g))


def _check_tree(view, base, model, keep, inherit):
    C, cap = base.max_size, cap_of(base.max_size)
    torch.cuda.synchronize()
    leaves = base._tree[:, cap:cap + C].cpu().numpy()
    got = view._tree.cpu().numpy()
    mx = 0.0
    for s in range(E):
        lv, kept = view_leaves(leaves[s], model.source[s], model.size[s], keep, inherit)
        assert np.array_equal(got[s], build_tree(lv, cap)), (s, inherit)
        mx = max(mx, float(lv.max()))
    assert view.max_priority == (mx if inherit else 1.0)
    assert torch.equal(view.totals, view._tree[:, 1]) and tuple(view.priority.shape) == (E, C)


@pytest.mark.parametrize("shape", ["small", "large"])
def test_the_view_tree_equals_the_pairwise_model(shape):
    base, model = _base(shape)
    for updated in (False, True):
        if updated:
            _update_base(base, 1)
        for inherit in (False, True):
            v = base.view(KEEP, inherit=inherit)
            assert v.state is base.state and v.size_s is base.size_s and v._tree is not base._tree
            _check_tree(v, base, model, KEEP, inherit)
    assert base.max_priority > 1.0  # the updates raised it; the views without inherit stayed at 1


@pytest.mark.parametrize("shape", ["small", "large"])
def test_a_view_of_every_source_that_inherits_is_the_base_tree(shape):
    base, _ = _base(shape)
    assert torch.equal(base.view(range(K), inherit=True)._tree, base._tree)
    _update_base(base, 2)
    v = base.view(range(K), inherit=True)
    assert torch.equal(v._tree, base._tree) and v.max_priority == float(base.priority.max())


def test_draws_land_on_kept_rows_and_match_searchsorted():
    base, model = _base("small")
    v = base.view(KEEP)
    u = torch.tensor([US] * E, dtype=torch.float32)
    got = v.sample_indices(u).cpu().numpy()
    got_base = base.sample_indices(u).cpu().numpy()
    for s in range(E):
        n = int(model.size[s])
        lv, kept = view_leaves(np.ones(base.max_size, dtype=F), model.source[s], n, KEEP, False)
        first = int(np.flatnonzero(kept)[0])
        for j, x in enumerate(US):
            assert kept[got[s, j]], (s, x)
            assert got[s, j] == (first if x == 0 else searchsorted_left(lv[:n], x)), (s, x)
            # the base buffer: every leaf 1, the unchanged behaviour (u == 0: slot 0)
            assert got_base[s, j] == searchsorted_left(np.ones(n), x), (s, x)
    assert not view_leaves(np.ones(base.max_size), model.source[1], int(model.size[1]), KEEP, False)[1][0]


def test_fifty_rounds_on_a_view_never_touch_a_foreign_row():
    base, model = _base("small")
    _update_base(base, 3)
    v = base.view(KEEP, batch_size=4)
    C, cap = base.max_size, cap_of(base.max_size)
    tree0, maxp0 = base._tree.clone(), base._maxp.clone()
    keep = torch.tensor(KEEP, device="cuda")
    rows = torch.arange(E, device="cuda")[:, None]
    g = torch.Generator(device="cuda").manual_seed(4)
    prio = lambda: 1.0 + 4.0 * torch.rand(E * 4, device="cuda", generator=g)  # noqa: E731
    batch = v.sample()
    for r in range(50):
        if r % 3 == 0:
            v.update_priority(prio())
            batch = v.sample()
        elif r % 3 == 1:
            batch = v.update_priority_and_sample(prio())
        else:
            td = 6.0 * torch.rand((E * 4, 2), device="cuda", generator=g)
            batch = v.update_priority_and_sample_td(td, 0.4, 1.0, v.ind, None)
        idx = v.ind.long()
        assert tuple(idx.shape) == (E, 4)
        assert bool(torch.isin(base.source[rows, idx], keep).all()), r
        for k, name in enumerate(ROWS):
            assert torch.equal(batch[k].view(E, 4, -1), getattr(base, name)[rows, idx]), (r, name)
    torch.cuda.synchronize()
    assert torch.equal(base._tree, tree0) and torch.equal(base._maxp, maxp0)
    leaves = v.priority.cpu().numpy()
    got = v._tree.cpu().numpy()
    moved = 0
    for s in range(E):
        kept = view_leaves(leaves[s], model.source[s], model.size[s], KEEP, True)[1]
        assert not leaves[s][~kept].any(), s  # every foreign leaf is still exactly 0
        assert (leaves[s][kept] > 0).all()
        moved += int((leaves[s][kept] != 1).sum())
        assert np.array_equal(got[s], build_tree(leaves[s], cap)), s
    assert moved > 0 and v.max_priority > 1.0


def test_views_refuse_empty_strata_and_inserts_and_rebuild_after_a_base_insert():
    base, model = _base("small")
    with pytest.raises(ValueError, match="strata"):
        base.view([K + 3])
    c = _calls("small")[0]
    # source 1 has rows in strata 0 and 2 only
    assert all((model.source[s, :model.size[s]] == 1).any() for s in (0, 2))
    with pytest.raises(ValueError, match=r"strata \[1\]"):
        base.view([1])
    v = base.view(KEEP)
    t = {k: torch.as_tensor(x, device="cuda") for k, x in c.items()}
    for call in (lambda: v.add_batch(*[t[k] for k in ARGS]), lambda: v.add_batch_ref(*[t[k] for k in ARGS]),
                 lambda: v.add(c["state"][0], c["action"][0], c["next_state"][0], 0.0, False, 0),
                 lambda: v.load_dataset(**{k: c[k] for k in ARGS[:6]}), v.reset_buffer):
        with pytest.raises(ValueError, match="view"):
            call()
    # one more row of source 0 into stratum 1: not in the snapshot, in the rebuilt view
    slot = int(model.size[1])
    one = [t[k][:1] for k in ARGS[:5]] + [torch.ones(1, dtype=torch.int32, device="cuda")]
    base.add_batch(*one, source=torch.zeros(1, dtype=torch.int32, device="cuda"))
    model.add_batch(np.array([1]), None, np.array([0], dtype=np.int32))
    torch.cuda.synchronize()
    assert float(v.priority[1, slot]) == 0.0 and float(base.priority[1, slot]) == 1.0
    assert v.rebuild() is v
    assert float(v.priority[1, slot]) == 1.0
    _check_tree(v, base, model, KEEP, False)
