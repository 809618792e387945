"""Datasets in and out of the LAP replay (exo_amd/replay.py load_dataset /
export_dataset, Agent.save_dataset / load_dataset): 8 strata, capacity 32,
80 / 7 dims."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, C, S, A = 8, 32, 80, 7
MAX_ACTION = 2.5
COUNTS = (30, 25, 20, 20, 20, 15, 12, 8)  # 150 rows, uneven, none above the capacity
ROWS = ("state", "action", "next_state", "reward", "not_done")


def _lap():
    from exo_amd.replay import LAP
    return LAP(S, A, "cuda", E, max_size=C, batch_size=4, max_action=MAX_ACTION)


def _dataset(counts, seed=0):
    rng = np.random.default_rng(seed)
    strata = rng.permutation(np.repeat(np.arange(len(counts)), counts)).astype(np.int32)
    n = strata.size
    return dict(state=rng.normal(0, 1, (n, S)).astype(np.float32),
                action=rng.uniform(-MAX_ACTION, MAX_ACTION, (n, A)).astype(np.float32),
                next_state=rng.normal(0, 1, (n, S)).astype(np.float32),
                reward=rng.uniform(-2, 3, n).astype(np.float32), done=rng.uniform(0, 1, n) < 0.1, strata=strata)


def _ulp(x):
    """The spacing of fp32 around x (the wider side at a power of two)."""
    inf = torch.full_like(x, np.inf)
    return torch.maximum((torch.nextafter(x, inf) - x).abs(), (torch.nextafter(x, -inf) - x).abs())


def _same_storage(a, b):
    torch.cuda.synchronize()
    for name in ROWS:
        assert torch.equal(getattr(a, name)[:, :C], getattr(b, name)[:, :C]), name
    assert torch.equal(a.ptr_s, b.ptr_s) and torch.equal(a.size_s, b.size_s)
    assert torch.equal(a._tree, b._tree) and float(a._maxp) == float(b._maxp)


def test_a_load_equals_add_batch_chunk_by_chunk():
    d = _dataset(COUNTS)
    a, b = _lap(), _lap()
    a.load_dataset(**d, chunk=64)
    t = {k: torch.as_tensor(v, device="cuda") for k, v in d.items()}
    for lo in range(0, 150, 64):
        b.add_batch(*[t[k][lo:lo + 64] for k in ("state", "action", "next_state", "reward", "done", "strata")])
    _same_storage(a, b)
    assert a.size_s.tolist() == list(COUNTS) and a.ptr_s.tolist() == list(COUNTS)
    for s, n in enumerate(COUNTS):
        leaves = a.priority[s]
        assert torch.equal(leaves[:n], torch.full((n,), a.max_priority, device="cuda")) and not leaves[n:].any()
        rows = np.nonzero(d["strata"] == s)[0]
        assert torch.equal(a.state[s, :n].cpu(), torch.as_tensor(d["state"][rows]))
        act = torch.as_tensor(d["action"][rows]) / MAX_ACTION
        assert bool(((a.action[s, :n].cpu() - act).abs() <= _ulp(act)).all())
        assert torch.equal(a.not_done[s, :n, 0].cpu(), torch.as_tensor(1.0 - d["done"][rows].astype(np.float32)))
    # torch inputs on the device, one chunk: the same buffer
    c = _lap()
    c.load_dataset(**t)
    _same_storage(a, c)


def test_a_load_of_more_rows_than_a_stratum_holds_keeps_the_newest():
    counts = (75, 40, 33, 32, 5, 5, 5, 5)
    d = _dataset(counts, seed=1)
    a = _lap()
    a.load_dataset(**d)  # one chunk by rows: split where a ring would wrap onto itself
    torch.cuda.synchronize()
    assert a.size_s.tolist() == [min(n, C) for n in counts]
    assert a.ptr_s.tolist() == [n % C for n in counts]
    out = a.export_dataset()
    for s, n in enumerate(counts):
        rows = np.nonzero(d["strata"] == s)[0][-C:]  # the newest, oldest first
        got = out["strata"] == s
        assert int(got.sum()) == len(rows)
        assert torch.equal(out["state"][got], torch.as_tensor(d["state"][rows])), s
        assert torch.equal(out["reward"][got], torch.as_tensor(d["reward"][rows])), s
        assert torch.equal(out["done"][got].bool(), torch.as_tensor(d["done"][rows])), s


def test_export_then_load_round_trips():
    counts = (75, 40, 33, 32, 5, 5, 5, 5)
    d = _dataset(counts, seed=2)
    a, b = _lap(), _lap()
    a.load_dataset(**d)
    out = a.export_dataset()
    assert set(out) == {"state", "action", "next_state", "reward", "done", "strata"}
    assert all(not t.is_cuda for t in out.values())
    # de-normalised actions: within 1 ulp of the dataset's
    for s in range(E):
        rows = np.nonzero(d["strata"] == s)[0][-C:]
        ref = torch.as_tensor(d["action"][rows])
        got = out["action"][out["strata"] == s]
        assert bool(((got - ref).abs() <= _ulp(ref)).all()), s
    b.load_dataset(**out)
    torch.cuda.synchronize()
    assert torch.equal(a.size_s, b.size_s)
    again = b.export_dataset()
    for k in ("state", "next_state", "reward", "done", "strata"):
        assert torch.equal(out[k], again[k]), k
    # normalised again: the stored actions within 1 ulp of the first buffer's
    na, nb = out["action"] / MAX_ACTION, again["action"] / MAX_ACTION
    assert bool(((nb - na).abs() <= _ulp(na)).all())
    # the unwrapped strata hold the same storage rows
    for s in (3, 4, 5, 6, 7):
        n = counts[s]
        assert torch.equal(a.state[s, :n], b.state[s, :n]) and torch.equal(a.reward[s, :n], b.reward[s, :n])


def test_an_empty_stratum_is_refused():
    d = _dataset((30, 25, 20, 20, 20, 15, 12, 0))
    with pytest.raises(ValueError, match="strata"):
        _lap().load_dataset(**d)


def test_the_agent_saves_and_loads_a_dataset_file(tmp_path):
    from exo_amd.td7 import Agent, Hyperparameters
    hp = Hyperparameters(batch_size=4)
    d = _dataset(COUNTS, seed=3)
    ags = [Agent(S, A, MAX_ACTION, offline=True, hp=hp, env_num=E, buffer_size=C) for _ in range(2)]
    ags[0].replay_buffer.load_dataset(**d)
    path = str(tmp_path / "dataset.pt")
    ags[0].save_dataset(path)
    ags[1].load_dataset(path)
    a, b = ags[0].replay_buffer, ags[1].replay_buffer
    torch.cuda.synchronize()
    assert torch.equal(a.size_s, b.size_s) and torch.equal(a.ptr_s, b.ptr_s)
    for name in ("state", "next_state", "reward", "not_done"):
        assert torch.equal(getattr(a, name)[:, :C], getattr(b, name)[:, :C]), name
    assert bool(((a.action - b.action).abs() <= _ulp(a.action)).all())
    assert torch.equal(a._tree, b._tree)
