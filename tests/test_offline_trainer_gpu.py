"""exo_amd.OfflineTrainer: offline TD7+BC training steps on a loaded dataset
as graph replays.

hp.batch_size = 5 over 8 strata (B = 40), target_update_rate = 4, a replay of
8 x 32 slots holding a seeded dataset of 8 x 24 rows, fp32 and bf16, 10 steps:
two target refreshes and five actor updates fall inside, and with
warmup_eager = 2 eight of the steps are graph replays.

* use_graphs=True equals use_graphs=False bit for bit: every net's weights, the
  Adam state, the tree leaves, max_priority, training_steps.
* Both equal a plain loop of Agent.train() on an identically seeded agent, bit
  for bit.  OfflineTrainer's priority update + next sample is the fused launch
  (LAP.update_priority_and_sample) where Agent.train() runs LAP.update_priority
  and LAP.sample; tests/test_lap_update_sample_chain_gpu.py holds that launch
  to the two launches bit for bit (tree, max_priority, indices, rows, RNG
  counter), so no tolerance is needed here either.
* release_graphs() at the end; a data-parallel agent is refused.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, C, ROWS_PER, STEPS = 8, 32, 24, 10
NETS = ("actor", "critic", "encoder", "actor_target", "critic_target", "fixed_encoder", "fixed_encoder_target")


def _dataset():
    rng = np.random.default_rng(11)
    n = E * ROWS_PER
    return dict(state=rng.normal(0, 1, (n, 80)).astype(np.float32),
                action=rng.uniform(-1, 1, (n, 7)).astype(np.float32),
                next_state=rng.normal(0, 1, (n, 80)).astype(np.float32),
                reward=rng.uniform(-2, 3, n).astype(np.float32), done=rng.uniform(0, 1, n) < 0.1,
                strata=rng.permutation(np.repeat(np.arange(E), ROWS_PER)).astype(np.int32))


def _agent(precision):
    from exo_amd.td7 import Agent, Hyperparameters
    torch.manual_seed(21)
    hp = Hyperparameters(batch_size=5, target_update_rate=4)
    ag = Agent(80, 7, 1, offline=True, hp=hp, env_num=E, buffer_size=C, precision=precision, graph_safe=True)
    assert ag.learner.fused_train, getattr(ag.learner.fused, "train_error", "no fused passes")
    ag.replay_buffer.load_dataset(**_dataset())
    return ag


def _state(ag):
    L = ag.learner
    torch.cuda.synchronize()
    out = {f"{m}.{n}": p.detach().clone() for m in NETS for n, p in getattr(L, m).named_parameters()}
    for name in ("actor_optimizer", "critic_optimizer", "encoder_optimizer"):
        opt = getattr(L, name)
        for k in ("m", "v", "_step"):  # FlatAdam's flat state
            out[f"{name}.{k}"] = getattr(opt, k).detach().clone()
    out["leaves"] = ag.replay_buffer.priority.clone()
    out["max_priority"] = ag.replay_buffer._maxp.clone()
    out["q_bounds"] = torch.stack([L.max, L.min, L.max_target, L.min_target]).clone()
    out["training_steps"] = torch.tensor(L.training_steps)
    return out


def _same(a, b, what):
    assert set(a) == set(b)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: {bad[:6]} differ"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_replays_equal_the_eager_steps_and_the_train_loop(precision):
    from exo_amd import OfflineTrainer
    runs = {}
    for graphs in (True, False):
        ag = _agent(precision)
        t = OfflineTrainer(ag, use_graphs=graphs, warmup_eager=2)
        for _ in range(STEPS):
            t.step()
        runs[graphs] = _state(ag)
        assert t.refreshes == 2 and ag.learner.training_steps == STEPS
        if graphs:
            # (update_actor, slot) graphs and the refresh graph; 8 steps were replays
            assert set(t.graphs) == {(False, 0), (True, 1)} and t._refresh_graph is not None
            assert t.release_graphs() == 3 and not t.graphs
    _same(runs[True], runs[False], "graphs vs eager")
    ag = _agent(precision)
    for _ in range(STEPS):
        ag.train()
    _same(_state(ag), runs[False], "Agent.train() loop vs OfflineTrainer")
    # training moved the nets and the priorities
    fresh = _state(_agent(precision))
    assert not torch.equal(fresh["actor.l0.weight"], runs[True]["actor.l0.weight"])
    assert not torch.equal(fresh["leaves"], runs[True]["leaves"])


def test_a_data_parallel_agent_is_refused():
    from exo_amd import OfflineTrainer
    ag = _agent("bf16")
    ag.sync.world = 2
    try:
        with pytest.raises(ValueError, match="one GPU"):
            OfflineTrainer(ag)
    finally:
        ag.sync.world = 1
