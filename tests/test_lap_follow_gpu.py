"""Live views (LAP.view(..., live=True), lap_views_follow) against the numpy
model of tests/lap_follow_model.py: after every add_batch, and after priority
updates on kept slots, every view's whole tree, max_priority, kept and ready()
equal the model's bit for bit.

Small: 3 strata of 13 slots (cap 16: every level in LDS), 14 calls of 9 rows;
strata 0 and 1 wrap (3 and 1 inserts cross the ring end), stratum 2 ends at 10
rows, 9 (call, stratum) pairs insert nothing and views [0] and [1, 3] each lose
16 kept rows to foreign ones (tests/test_lap_follow_model_host.py pins this).
Large: 2 strata of 5,000 slots (cap 8,192 = TOPN: one level in global memory),
20 calls of 700 rows, both rings cross their end once."""
import functools

import numpy as np
import pytest
import torch

from lap_follow_model import Follow
from lap_view_model import F, make_calls

pytestmark = pytest.mark.gpu

S, A, B = 5, 2, 4
KEEPS = ([0], [1, 3], [0, 1, 2, 3])
ARGS = ("state", "action", "next_state", "reward", "done", "strata", "active")
ROWS = ("state", "action", "next_state", "reward", "not_done")
SETS = dict(small=dict(E=3, C=13, calls=(11, 3, 5, 2, 14, 9, [0.6, 0.3, 0.1], 4)),
            large=dict(E=2, C=5000, calls=(12, 2, 5, 2, 20, 700, [0.5, 0.5], 4)))


@functools.lru_cache(maxsize=None)
def _calls(name):
    return make_calls(*SETS[name]["calls"])


def _lap(E, C):
    from exo_amd.replay import LAP
    return LAP(S, A, "cuda", E, max_size=C, batch_size=B)


def _add(base, c, source=True):
    t = {k: torch.as_tensor(v, device="cuda") for k, v in c.items()}
    base.add_batch(*[t[k] for k in ARGS], source=t["source"] if source else None)


def _check(views, model, where):
    torch.cuda.synchronize()
    for k, v in enumerate(views):
        m = model.views[k]
        assert np.array_equal(v._tree.cpu().numpy(), model.tree(k)), (where, k)
        assert v.max_priority == float(m.maxp), (where, k)
        assert v.kept.cpu().tolist() == m.kept.tolist(), (where, k)
        assert v.ready() == m.ready(), (where, k)


def _update(views, model, rng, where):
    """update_priority on every view the model calls ready: B kept slots per
    stratum from the model (duplicates happen: the last one wins), non-integer
    priorities.  Returns the views updated."""
    done = []
    for k, v in enumerate(views):
        m = model.views[k]
        if not m.ready():
            continue
        idx = np.stack([rng.choice(np.flatnonzero(m.leaves[s] > 0), B) for s in range(model.E)]).astype(np.int32)
        prio = rng.uniform(0.25, 6.0, (model.E, B)).astype(F)
        v.update_priority(torch.as_tensor(prio, device="cuda"), ind=torch.as_tensor(idx, device="cuda"))
        model.on_update(k, idx, prio)
        done.append(k)
    _check(views, model, where)
    return done


def _follow(name, updates):
    """The call set into a buffer with the three live views (taken while it is
    empty) and into a twin without views; checks after every call."""
    sh = SETS[name]
    base, twin = _lap(sh["E"], sh["C"]), _lap(sh["E"], sh["C"])
    twin.enable_sources()
    views = [base.view(k, live=True) for k in KEEPS]
    model = Follow(sh["E"], sh["C"], KEEPS)
    assert base.live_generation == 3 and not any(v.ready() for v in views)
    _check(views, model, "empty")
    rng = np.random.default_rng(3)
    n_upd = [0] * len(KEEPS)
    for j, c in enumerate(_calls(name)):
        _add(base, c)
        _add(twin, c)
        model.add_batch(c["strata"], c["active"], c["source"])
        _check(views, model, ("insert", j))
        if updates:
            for k in _update(views, model, rng, ("update", j)):
                n_upd[k] += 1
    assert base.insert_epoch == len(_calls(name))
    # the base is the buffer it would be without views
    C = sh["C"]
    for nm in ROWS:
        assert torch.equal(getattr(base, nm)[:, :C], getattr(twin, nm)[:, :C]), nm
    assert torch.equal(base.source[:, :C], twin.source[:, :C])
    assert torch.equal(base._tree, twin._tree) and torch.equal(base._maxp, twin._maxp)
    assert torch.equal(base.ptr_s, twin.ptr_s) and torch.equal(base.size_s, twin.size_s)
    assert np.array_equal(base.source[:, :C].cpu().numpy(), model.rings.source)
    return base, views, model, n_upd


def test_small_trees_follow_inserts_and_keep_updates():
    _, views, model, n_upd = _follow("small", True)
    assert min(n_upd) >= 10, n_upd
    assert all(float(v.maxp) > 1 for v in model.views)
    assert [v.lost for v in model.views[:2]] == [16, 16]


def test_global_level_trees_follow_inserts_and_keep_updates():
    from exo_amd.replay import LAP  # noqa: F401
    base, views, model, n_upd = _follow("large", True)
    assert 2 * base._cap > 8192  # TOPN: the lowest level is recomputed in global memory
    assert min(n_upd) >= 10, n_upd
    assert model.wraps.tolist() == [1, 1]


def test_a_followed_view_equals_a_rebuilt_one():
    base, views, model, _ = _follow("small", False)
    assert all(v.ready() for v in model.views)
    for keep, v in zip(KEEPS, views):
        fresh = base.view(keep)
        assert not fresh.live and torch.equal(v._tree, fresh._tree) and torch.equal(v._maxp, fresh._maxp)
        assert torch.equal(v.kept, fresh.kept)
    assert base.live_generation == 3 and len(base._live) == 3


def test_inherit_views_follow_from_an_empty_and_a_part_filled_buffer():
    """view(keep, inherit=True, live=True): taken from the empty buffer it starts
    at max_priority 1 (the inherit build's maximum over no kept leaf would be 0
    and every later row would enter at leaf 0: never ready); taken later it
    starts from the base's updated leaves and their maximum.  Both then follow
    at their own max_priority."""
    sh = SETS["small"]
    base = _lap(sh["E"], sh["C"])
    model = Follow(sh["E"], sh["C"], [])
    views = [base.view([0], inherit=True, live=True)]
    model.attach([0], base.priority.cpu().numpy())
    _check(views, model, "empty")
    assert views[0].max_priority == 1.0 and not views[0].ready()
    assert views[0].rebuild() is views[0]  # still no row: the same again
    _check(views, model, "empty, rebuilt")
    rng = np.random.default_rng(5)
    g = torch.Generator(device="cuda").manual_seed(6)
    n_upd = [0, 0, 0]
    for j, c in enumerate(_calls("small")):
        _add(base, c)
        model.add_batch(c["strata"], c["active"], c["source"])
        _check(views, model, ("insert", j))
        if j == 4:
            # the base learns priorities of its own, then two more views inherit them
            # (slots 0..3 of every stratum are filled and hold rows of sources 1 / 3 and of source 2)
            first = torch.arange(B, device="cuda", dtype=torch.int32).repeat(sh["E"], 1)
            base.update_priority(1.5 + 4.0 * torch.rand(sh["E"] * B, device="cuda", generator=g), ind=first)
            torch.cuda.synchronize()
            leaves = base.priority.cpu().numpy()
            assert (leaves != 1)[leaves > 0].any() and base.max_priority > 1
            for keep in ([1, 3], [2]):
                views.append(base.view(keep, inherit=True, live=True))
                k = model.attach(keep, leaves)
                assert float(model.views[k].maxp) == float(model.views[k].leaves.max()) != 1.0
            _check(views, model, "part filled")
        for k in _update(views, model, rng, ("update", j)):
            n_upd[k] += 1
    # the model alone decides when a view is updated (every stratum keeps a row): after 11 of the 14 calls
    # for [0], after 10 and 3 of the 10 calls that [1, 3] and [2] (source 2 is rare in stratum 2) are there for
    assert all(v.ready() for v in views) and n_upd == [11, 10, 3], n_upd
    assert int(views[0].kept.sum()) > 0 and all(float(v.maxp) > 1 for v in model.views)


def test_sampling_stays_inside_the_view():
    sh = SETS["small"]
    base = _lap(sh["E"], sh["C"])
    views = [base.view(k, live=True) for k in KEEPS[:2]]
    model = Follow(sh["E"], sh["C"], KEEPS[:2])
    snap = None
    for j, c in enumerate(_calls("small")):
        _add(base, c)
        model.add_batch(c["strata"], c["active"], c["source"])
        if j == 5 and model.views[0].ready():
            snap = base.view(KEEPS[0])  # a snapshot: may name foreign rows by the end, not asserted on
    rows = torch.arange(sh["E"], device="cuda")[:, None]
    checked = 0
    for k, v in enumerate(views):
        if not model.views[k].ready():
            continue
        keep = torch.tensor(KEEPS[k], device="cuda", dtype=torch.int32)
        for r in range(50):
            batch = v.sample()
            idx = v.ind.long()
            assert bool(torch.isin(base.source[rows, idx], keep).all()), (k, r)
            assert torch.equal(batch[0].view(sh["E"], B, S), base.state[rows, idx])
        checked += 1
    assert checked == 2
    if snap is not None:
        snap.sample()
        torch.cuda.synchronize()


def _one(E, n, stratum, source, active=None, seed=0):
    rng = np.random.default_rng(seed)
    return dict(state=rng.normal(0, 1, (n, S)).astype(F), action=rng.uniform(-1, 1, (n, A)).astype(F),
                next_state=rng.normal(0, 1, (n, S)).astype(F), reward=rng.uniform(-2, 3, n).astype(F),
                done=np.zeros(n, dtype=bool), strata=np.asarray(stratum, dtype=np.int32),
                active=np.ones(n, dtype=bool) if active is None else np.asarray(active, dtype=bool),
                source=np.asarray(source, dtype=np.int32))


@pytest.mark.parametrize("C", [13, 2, 1])
def test_edges(C):
    E = 3
    base = _lap(E, C)
    views = [base.view(k, live=True) for k in KEEPS]
    model = Follow(E, C, KEEPS)

    def put(c, source=True, where=None):
        _add(base, c, source)
        model.add_batch(c["strata"], c["active"], c["source"] if source else None)
        _check(views, model, (C, where))

    # a partly filled ring first, so that the full insert below starts mid-ring
    n0 = max(C // 2, 1)
    put(_one(E, n0 + 1, [1] * n0 + [0], [0, 1, 2, 3, 0, 1, 2][:n0] + [1], seed=1), where="part")
    # exactly `capacity` active rows of stratum 1 (and an inactive one between them)
    src = [(3 * i + 1) % 4 for i in range(C + 1)]
    put(_one(E, C + 1, [1] * (C + 1), src, active=[True] + [False] + [True] * (C - 1), seed=2), where="full")
    assert model.rings.size[1] == C
    # no active row; then rows whose stratum is out of range next to real ones
    put(_one(E, 4, [0, 1, 2, 1], [0, 1, 2, 3], active=[False] * 4, seed=3), where="inactive")
    put(_one(E, 4, [E, 2, -1, 0], [0, 0, 1, 3], seed=4), where="bad stratum")
    # untagged rows (no source on a buffer that has the column) evict kept ones
    before = [int(v.kept.sum()) for v in model.views]
    put(_one(E, 3, [1, 0, 2], [0, 0, 0], seed=5), source=False, where="untagged")
    assert int(model.views[2].kept.sum()) < before[2]  # stratum 1 was full of kept rows
    put(_one(E, 3, [1, 2, 0], [0, 1, 3], seed=6), where="tagged again")
    # reset_buffer empties the attached views with the base; they follow on
    base.reset_buffer()
    model.reset()
    _check(views, model, (C, "reset"))
    assert not any(v.ready() for v in views)
    put(_one(E, 3, [0, 1, 2], [0, 1, 0], seed=7), where="after reset")
    assert views[2].ready() and not views[0].ready()


def test_launcher_rejects_bad_arguments():
    import ctypes

    from exo_amd import _native as nat
    base = _lap(2, 13)
    v = base.view([0], live=True)
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    d, st, tab, s = ctypes.byref(base._desc), ctypes.byref(base._store), nat.ptr(base._live_table), base._stream()
    f = nat.lib().lap_views_follow
    assert f(None, st, nat.ptr(ws), None, 4, tab, 1, s) == -22
    assert f(d, None, nat.ptr(ws), None, 4, tab, 1, s) == -22
    assert f(d, st, None, None, 4, tab, 1, s) == -22
    assert f(d, st, nat.ptr(ws), None, 4, None, 1, s) == -22
    assert f(d, st, nat.ptr(ws), None, 4, tab, 0, s) == -22
    assert f(d, st, nat.ptr(ws), None, -1, tab, 1, s) == -22
    bad = nat.LapTreeDesc(base._tree.data_ptr(), base._maxp.data_ptr(), 2, 13, 12)  # cap no power of two
    assert f(ctypes.byref(bad), st, nat.ptr(ws), None, 4, tab, 1, s) == -22
    tree0 = v._tree.clone()
    assert f(d, st, nat.ptr(ws), None, 0, tab, 1, s) == 0  # n == 0: nothing launched
    torch.cuda.synchronize()
    assert torch.equal(v._tree, tree0)


def test_stale_draws_detach_and_capture(monkeypatch):
    import ctypes

    from exo_amd import _native as nat
    sh = SETS["small"]
    calls = _calls("small")
    base = _lap(sh["E"], sh["C"])
    view = base.view(KEEPS[2], live=True)
    for c in calls[:6]:
        _add(base, c)
    assert view.ready() and not view.stale  # never sampled: nothing pending
    view.sample()
    assert not view.stale
    prio = torch.full((sh["E"] * B,), 2.5, device="cuda")
    view.update_priority(prio)  # a fresh draw: fine
    view.sample()
    _add(base, calls[6])
    assert view.stale
    for call in (lambda: view.update_priority(prio), lambda: view.update_priority_and_sample(prio),
                 lambda: view.update_priority_and_sample_td(torch.ones((sh["E"] * B, 2), device="cuda"), 0.4, 1.0,
                                                            view.ind, None)):
        with pytest.raises(ValueError, match="sample"):
            call()
    view.sample()
    assert not view.stale
    view.update_priority_and_sample(prio)
    assert not view.stale
    # a snapshot view never goes stale
    snap = base.view(KEEPS[2])
    snap.sample()
    _add(base, calls[7])
    assert not snap.stale and view.stale
    snap.update_priority(prio)
    # detach: later inserts leave the tree alone
    gen = base.live_generation
    assert view.detach() is view and not view.live and base.live_generation == gen + 1 and not base._live
    torch.cuda.synchronize()
    tree0, kept0 = view._tree.clone(), view.kept.clone()
    _add(base, calls[8])
    torch.cuda.synchronize()
    assert torch.equal(view._tree, tree0) and torch.equal(view.kept, kept0) and not view.stale
    view.rebuild()
    torch.cuda.synchronize()
    assert int(view.kept.sum()) == int(base.size_s.sum())
    # attaching while the stream captures is refused before anything is launched
    other = base.view([0], live=True)
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)  # no capture needed to see the refusal
        with pytest.raises(RuntimeError, match="capture"):
            base.view([1], live=True)
        with pytest.raises(RuntimeError, match="capture"):
            other.detach()
    assert base._live == [other] and other.live and base.live_generation == gen + 2
    # the 65th view is refused before anything of it is built or attached
    more = [base.view([0], live=True) for _ in range(base.MAX_LIVE_VIEWS - 1)]
    with pytest.raises(ValueError, match="at most 64"):
        base.view([0], live=True)
    assert len(base._live) == 64 and base._live[1:] == more
    # detached views leave zeroed entries behind them in the table
    for v in more:
        v.detach()
    torch.cuda.synchronize()
    entry = ctypes.sizeof(nat.LapViewEntry)
    assert base._live == [other] and not bool(base._live_table[entry:].any()) and bool(base._live_table[:entry].any())
