"""The LAP replay's behaviour-policy column (LAP.enable_sources, add_batch(source=),
lap_store_batch_src, lap_source_counts): 3 strata of 37 slots (cap 64), 4
sources, 80 / 7 and 6 / 3 dims (the float4 and the scalar row copy).

Five add_batch calls of 24 rows with inactive rows and one row of an
out-of-range stratum each: stratum 0 wraps, the others stay below capacity.
The reference for the column is the numpy ring model of tests/lap_view_model.py;
a twin buffer fed the same rows without source= must end with equal rows, tree,
ring state and max_priority.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

from lap_view_model import Rings, make_calls

pytestmark = pytest.mark.gpu

E, C, K = 3, 37, 4
PROBS = [0.6, 0.15, 0.25]
ROWS = ("state", "action", "next_state", "reward", "not_done")
ARGS = ("state", "action", "next_state", "reward", "done", "strata", "active")


def _lap(S, A):
    from exo_amd.replay import LAP
    return LAP(S, A, "cuda", E, max_size=C, batch_size=4, max_action=2.0)


@functools.lru_cache(maxsize=None)
def _calls(S, A):
    return make_calls(3, E, S, A, 5, 24, PROBS, K, bad_stratum=5)


def _dev(call):
    return {k: torch.as_tensor(v, device="cuda") for k, v in call.items()}


def _feed(lap, calls, tagged=True, untagged_calls=()):
    model = Rings(E, C)
    for j, c in enumerate(calls):
        t = _dev(c)
        tag = tagged and j not in untagged_calls
        lap.add_batch(*[t[k] for k in ARGS], **(dict(source=t["source"]) if tag else {}))
        model.add_batch(c["strata"], c["active"], c["source"] if tag else None)
    torch.cuda.synchronize()
    return model


def _same_buffer(a, b):
    for name in ROWS:
        assert torch.equal(getattr(a, name)[:, :C], getattr(b, name)[:, :C]), name
    assert torch.equal(a.ptr_s, b.ptr_s) and torch.equal(a.size_s, b.size_s)
    assert torch.equal(a._tree, b._tree) and torch.equal(a._maxp, b._maxp)


def _check_column(lap, model):
    assert lap.source.dtype == torch.int32 and tuple(lap.source.shape) == (E, C + 1)
    assert lap.size_s.tolist() == model.size.tolist() and lap.ptr_s.tolist() == model.ptr.tolist()
    # the filled slots hold the model's sources, every other live slot is still -1
    assert np.array_equal(lap.source[:, :C].cpu().numpy(), model.source)


@pytest.mark.parametrize("dims", [(80, 7), (6, 3)])
def test_add_batch_records_the_source_of_every_row(dims):
    calls = _calls(*dims)
    lap, twin = _lap(*dims), _lap(*dims)
    assert lap.source is None
    model = _feed(lap, calls)
    _feed(twin, calls, tagged=False)
    assert twin.source is None
    # the shape of the case: stratum 0 wrapped, stratum 1 and 2 below capacity
    given = np.concatenate([c["strata"][c["active"]] for c in calls])
    assert (given == 0).sum() > C and model.size[0] == C and 0 < model.size[1] < C and 0 < model.size[2] < C
    _check_column(lap, model)
    _same_buffer(lap, twin)
    assert lap.enable_sources() is lap.source  # idempotent


def test_a_call_without_source_on_a_tagged_buffer_writes_minus_one():
    calls = _calls(80, 7)
    lap, twin = _lap(80, 7), _lap(80, 7)
    model = _feed(lap, calls, untagged_calls=(1, 4))
    _feed(twin, calls, tagged=False)
    assert (model.source[:, :] == -1).sum() > (E * C - model.size.sum())  # some filled slots are untagged
    _check_column(lap, model)
    _same_buffer(lap, twin)
    t = _dev(calls[0])
    with pytest.raises(ValueError, match="source column"):
        lap.add(calls[0]["state"][0], calls[0]["action"][0], calls[0]["next_state"][0], 0.0, False, 0)
    with pytest.raises(ValueError, match="source column"):
        lap.add_batch_ref(*[t[k] for k in ARGS])
    with pytest.raises(ValueError, match="int32"):
        lap.add_batch(*[t[k] for k in ARGS], source=t["source"].long())
    torch.cuda.synchronize()
    _check_column(lap, model)  # the refused calls wrote nothing


def test_export_then_load_keeps_the_column():
    calls = _calls(80, 7)
    a, b, c = _lap(80, 7), _lap(80, 7), _lap(80, 7)
    model = _feed(a, calls, untagged_calls=(2,))
    out = a.export_dataset()
    assert out["source"].dtype == torch.int32 and not out["source"].is_cuda
    # oldest first per stratum
    want = np.concatenate([model.source[s, (model.ptr[s] - model.size[s] + np.arange(model.size[s])) % C]
                           for s in range(E)])
    assert np.array_equal(out["source"].numpy(), want)
    b.load_dataset(**out)
    torch.cuda.synchronize()
    again = b.export_dataset()
    for k in ("state", "next_state", "reward", "done", "strata", "source"):
        assert torch.equal(out[k], again[k]), k
    for s in range(E):
        n = int(model.size[s])
        assert np.array_equal(b.source[s, :n].cpu().numpy(), want[out["strata"].numpy() == s])
        assert bool((b.source[s, n:C] == -1).all())
    # a dataset without the key loads as before, into a buffer without the column
    del out["source"]
    c.load_dataset(**out)
    assert c.source is None and torch.equal(c.size_s, b.size_s) and torch.equal(c.state[:, :C], b.state[:, :C])
    assert torch.equal(c._tree, b._tree)


def test_source_counts_equal_bincount():
    calls = _calls(80, 7)
    lap = _lap(80, 7)
    model = _feed(lap, calls, untagged_calls=(3,))
    got = lap.source_counts(K)
    assert got.dtype == torch.int64 and tuple(got.shape) == (E, K + 1)
    want = np.zeros((E, K + 1), dtype=np.int64)
    for s in range(E):
        src = model.source[s, :model.size[s]]
        want[s, :K] = np.bincount(src[src >= 0], minlength=K)
        want[s, K] = (src < 0).sum()
    assert want[:, K].sum() > 0 and np.array_equal(got.cpu().numpy(), want)
    assert int(got.sum()) == int(model.size.sum())
    with pytest.raises(ValueError, match="source column"):
        _lap(80, 7).source_counts(K)
