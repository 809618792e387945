"""Offline training on a view (Agent.use_replay(base.view([p])) + OfflineTrainer):
8 strata of 32 slots holding a seeded dataset of 8 x 24 rows tagged with 3
sources (no wrap), hp.batch_size = 5, bf16.

* The first step on the view equals the first step on a compact buffer: a
  fresh replay loaded with source p's rows alone, in the same order, under the
  same torch seed (the DeviceRNG streams follow it).  Every priority is 1, so
  both draw the same j-th kept row: the first batches are equal row for row
  and after one OfflineTrainer.step() every learner parameter is equal bit for
  bit.  (Later steps may differ: the trees have different shapes.)
* 12 steps as graph replays on the view: every sampled index is a kept row and
  every foreign leaf is still 0 at the end.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, C, ROWS_PER, K, P = 8, 32, 24, 3, 1
NETS = ("actor", "critic", "encoder", "actor_target", "critic_target", "fixed_encoder", "fixed_encoder_target")


def _dataset():
    rng = np.random.default_rng(13)
    n = E * ROWS_PER
    return dict(state=rng.normal(0, 1, (n, 80)).astype(np.float32),
                action=rng.uniform(-1, 1, (n, 7)).astype(np.float32),
                next_state=rng.normal(0, 1, (n, 80)).astype(np.float32),
                reward=rng.uniform(-2, 3, n).astype(np.float32), done=rng.uniform(0, 1, n) < 0.1,
                strata=rng.permutation(np.repeat(np.arange(E), ROWS_PER)).astype(np.int32),
                source=rng.integers(0, K, n).astype(np.int32))


def _base():
    from exo_amd.replay import LAP
    base = LAP(80, 7, "cuda", E, max_size=C, batch_size=5)
    base.load_dataset(**_dataset())
    return base


def _agent(buffer_size):
    from exo_amd.td7 import Agent, Hyperparameters
    torch.manual_seed(21)
    hp = Hyperparameters(batch_size=5, target_update_rate=4)
    ag = Agent(80, 7, 1, offline=True, hp=hp, env_num=E, buffer_size=buffer_size, precision="bf16", graph_safe=True)
    assert ag.learner.fused_train, getattr(ag.learner.fused, "train_error", "no fused passes")
    return ag


def _params(ag):
    torch.cuda.synchronize()
    return {f"{m}.{n}": p.detach().clone() for m in NETS for n, p in getattr(ag.learner, m).named_parameters()}


def test_the_first_step_on_a_view_equals_the_first_step_on_a_compact_buffer():
    from exo_amd import OfflineTrainer
    base = _base()
    a = _agent(1)
    own = a.replay_buffer
    view = a.use_replay(base.view([P]))
    assert a.replay_buffer is view and own.max_size == 1
    b = _agent(C)
    d = _dataset()
    mine = d.pop("source") == P
    b.replay_buffer.load_dataset(**{k: v[mine] for k, v in d.items()})
    ta, tb = OfflineTrainer(a, use_graphs=False), OfflineTrainer(b, use_graphs=False)
    ta.step()
    tb.step()
    torch.cuda.synchronize()
    # the first batch (slot 0; the step sampled the next one into slot 1)
    (ba, ia), (bb, ib) = view._slot(0), b.replay_buffer._slot(0)
    for x, y in zip(ba, bb):
        assert torch.equal(x, y)
    # the j-th kept slot of the view is slot j of the compact buffer
    kept = (base.source[:, :C] == P)
    rank = (kept.cumsum(1) - 1)[torch.arange(E, device="cuda")[:, None], ia.long()]
    assert bool(kept[torch.arange(E, device="cuda")[:, None], ia.long()].all()) and torch.equal(rank.int(), ib)
    pa, pb = _params(a), _params(b)
    bad = [k for k in pa if not torch.equal(pa[k], pb[k])]
    assert not bad, bad[:6]
    fresh = _params(_agent(1))
    assert any(not torch.equal(fresh[k], pa[k]) for k in pa)  # the step moved the nets


def test_twelve_graph_steps_on_a_view_stay_inside_it():
    from exo_amd import OfflineTrainer
    base = _base()
    tree0 = base._tree.clone()
    a = _agent(1)
    view = a.use_replay(base.view([P]))
    t = OfflineTrainer(a, use_graphs=True, warmup_eager=2)
    kept = (base.source[:, :C] == P)
    rows = torch.arange(E, device="cuda")[:, None]
    for _ in range(12):
        t.step()
        for slot in (0, 1):
            assert bool(kept[rows, view._slot(slot)[1].long()].all())
    assert t.graphs and a.learner.training_steps == 12 and t.refreshes == 3
    assert t.release_graphs() == 3 and not t.graphs  # retire_graphs(t)
    leaves = view.priority
    assert not bool(leaves[~kept].any()) and bool((leaves[kept] > 0).all()) and bool((leaves[kept] != 1).any())
    assert torch.equal(base._tree, tree0)


def test_use_replay_checks_the_replay():
    from exo_amd.replay import LAP
    a = _agent(1)
    with pytest.raises(ValueError, match="use_replay"):
        a.use_replay(LAP(80, 7, "cuda", E, max_size=C, batch_size=4))
    with pytest.raises(ValueError, match="use_replay"):
        a.use_replay(LAP(80, 7, "cuda", E + 1, max_size=C, batch_size=5))
    a.sync.world = 2
    try:
        with pytest.raises(ValueError, match="one GPU"):
            a.use_replay(_base())
    finally:
        a.sync.world = 1
