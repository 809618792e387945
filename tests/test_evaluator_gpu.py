"""exo_amd.Evaluator: every policy of a PolicySet evaluated for one episode in
its own segment of one VecExoskeletonEnv, one td7f_select_multi launch per step.

The reference is a hand-written loop on a second env with the same seed whose
actions come from single-policy td7f_select launches (sigma = 0) on the row
slices: those are bit-equal to the multi-policy launch
(tests/test_select_multi_gpu.py) and the env is deterministic, so counters,
returns, step counts and done flags must be exactly equal.

Env draws are Philox blocks keyed by (seed, env, episode) (csrc/exo_env.hip
Draws / exo_reset_kernel: `Draws{draws, seed, env, episode}`), so env i's
episode does not depend on how many envs the context holds: policy 0's result
in a K = 2 evaluator equals a K = 1 evaluator of policy 0 alone with the same
seed, which test_per_policy_env_arguments checks directly.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import select_full_perturb
from test_select_full_gpu import _perturb_on_device

pytestmark = pytest.mark.gpu

SEQS = ([1, 0, 1, 0, 0, 0, 0], [0, 1, 1, 1, 0, 0, 0])


@functools.lru_cache(maxsize=None)
def _agent(precision, k):
    from exo_amd.td7 import Agent, Hyperparameters
    torch.manual_seed(500 + k)
    ag = Agent(80, 7, 1, hp=Hyperparameters(), env_num=8, device="cuda", buffer_size=64, precision=precision)
    _perturb_on_device(ag.learner.actor, 9000 + 100 * k, select_full_perturb)
    _perturb_on_device(ag.learner.fixed_encoder, 9050 + 100 * k, select_full_perturb)
    return ag


def _agent_state(ag):
    L = ag.learner
    return (L.exploration_noise_t.clone(), L._explore_rng.state.clone(), L.training_steps,
            int(ag.replay_buffer.size_s.sum()))


def _same_state(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]


def _single(ag, obs):
    """the agent's live policy through its own td7f_select, sigma = 0; noise state restored"""
    L = ag.learner
    sig, rng = L.exploration_noise_t.clone(), L._explore_rng.state.clone()
    L.exploration_noise_t.fill_(0.0)
    a = L.fused.select(obs, rt=1).clone()
    L.exploration_noise_t.copy_(sig)
    L._explore_rng.state.copy_(rng)
    return a


def _hand_loop(agents, per, seed, **env_kw):
    from exo_amd import VecExoskeletonEnv
    n = per * len(agents)
    env = VecExoskeletonEnv(n, motions=np.tile(np.arange(per) % 8, len(agents)), seed=seed, device="cuda", **env_kw)
    out = env.new_outputs(True)
    obs = env.reset(obs_out=out[0])
    done = out[2]
    counters = torch.zeros((n, 5), dtype=torch.float32, device="cuda")
    ret = torch.zeros(n, dtype=torch.float32, device="cuda")
    steps = torch.zeros(n, dtype=torch.float32, device="cuda")
    out[1].zero_()
    for _ in range(env.max_len):
        active = done == 0
        a = torch.cat([_single(ag, obs[per * p:per * (p + 1)].contiguous()) for p, ag in enumerate(agents)])
        _, rew, _, info = env.step(a, active=active, out=out)
        counters = env.eval_metrics(info, stepped=active, counters=counters)
        ret += rew * active.float()
        steps += active.float()
    torch.cuda.synchronize()
    res = (counters.cpu().numpy(), ret.cpu().numpy(), steps.cpu().numpy(), done.cpu().numpy().copy())
    env.close()
    return res


def _arrays(ev):
    torch.cuda.synchronize()
    return (ev.counters.cpu().numpy(), ev.returns.cpu().numpy(), ev.steps.cpu().numpy(),
            ev._out[2].cpu().numpy().copy())


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_evaluator_equals_the_hand_written_loop(precision, graph):
    from exo_amd import Evaluator
    from exo_amd.fused import PolicySet
    agents = [_agent(precision, 0), _agent(precision, 1)]
    ev = Evaluator(PolicySet.from_agents(agents, use_checkpoint=False), [8, 8], seed=3, graph=graph)
    try:
        res = ev.evaluate()
        got = _arrays(ev)
    finally:
        ev.close()
    want = _hand_loop(agents, 8, 3)
    for g, w, what in zip(got, want, ("counters", "returns", "steps", "done")):
        np.testing.assert_array_equal(g, w, err_msg=what)
    assert want[3].all() and want[2].min() > 3
    names = ("all_axes_suppressed", "any_axis_suppressed", "ampl_total_neg", "ampl_total_nonneg", "ampl_total_neg_sum")
    for p in range(2):
        r, s = res[p], slice(8 * p, 8 * p + 8)
        assert r["env_steps"] == int(want[2][s].sum()) and r["envs"] == 8
        assert r["return_mean"] == float(want[1][s].astype(np.float64).mean())
        assert r["return_min"] == float(want[1][s].min())
        for j, name in enumerate(names):
            assert r[name] == float(want[0][s, j].astype(np.float64).sum())
    assert res[0]["return_mean"] != res[1]["return_mean"]


def test_repeat_evaluation_and_untouched_agents():
    from exo_amd import Evaluator, graphs
    from exo_amd.fused import PolicySet
    agents = [_agent("bf16", 0), _agent("bf16", 1)]
    before = [_agent_state(a) for a in agents]
    kept = graphs.kept_graphs()
    ev = Evaluator(PolicySet.from_agents(agents, use_checkpoint=True), [8, 8], seed=5, graph=True)
    try:
        first = ev.evaluate(episodes=1)
        assert graphs.kept_graphs() == kept + 1
        second = ev.evaluate(episodes=1)
        assert first == second
        for r in first:
            for k in ("occurrence", "total", "torque_any", "torque_all"):
                assert len(r[k]) == 2 and np.isfinite(r[k]).all()
        # the checkpoint nets are other weights than the live ones
        live = Evaluator(PolicySet.from_agents(agents, use_checkpoint=False), [8, 8], seed=5, graph=False)
        assert live.evaluate()[0]["return_mean"] != first[0]["return_mean"]
        live.close()
    finally:
        assert ev.release() == 1
        assert graphs.kept_graphs() == kept
        ev.close()
    torch.cuda.synchronize()
    assert all(_same_state(b, _agent_state(a)) for a, b in zip(agents, before))


def test_per_policy_env_arguments():
    from exo_amd import Evaluator
    from exo_amd.fused import PolicySet
    agents = [_agent("bf16", 0), _agent("bf16", 1)]
    per = [dict(tremor_sequence=s) for s in SEQS]
    ev = Evaluator(PolicySet.from_agents(agents, use_checkpoint=False), [8, 8], per_policy_env_kwargs=per, seed=9,
                   env_kwargs=dict(max_force_elbow=25.0), graph=False)
    one = Evaluator(PolicySet.from_agents(agents[:1], use_checkpoint=False), [8], per_policy_env_kwargs=per[:1],
                    seed=9, env_kwargs=dict(max_force_elbow=25.0), graph=False)
    try:
        np.testing.assert_array_equal(ev.env.tremor_sequence[:8], np.tile(SEQS[0], (8, 1)))
        np.testing.assert_array_equal(ev.env.tremor_sequence[8:], np.tile(SEQS[1], (8, 1)))
        np.testing.assert_array_equal(ev.env.motions, np.tile(np.arange(8), 2))
        both, alone = ev.evaluate(episodes=1), one.evaluate(episodes=1)
        assert both[0] == alone[0]
        assert both[1]["return_mean"] != both[0]["return_mean"]
    finally:
        ev.close()
        one.close()
    with pytest.raises(ValueError, match="every policy"):
        Evaluator(PolicySet.from_agents(agents, use_checkpoint=False), [8, 8],
                  per_policy_env_kwargs=[dict(tremor_sequence=SEQS[0]), {}])


@pytest.mark.parametrize("use_graphs", [False, True])
def test_offline_trainer_evaluate_follows_the_training(use_graphs):
    """OfflineTrainer.evaluate reports the live policy as trained so far: the
    HIP optimiser (and, with graphs, replays) move the actor without moving a
    torch version counter, so the kept evaluator must repack at every call."""
    from exo_amd import Evaluator, OfflineTrainer
    from test_offline_trainer_gpu import _agent as offline_agent
    ag = offline_agent("bf16")
    L = ag.learner
    t = OfflineTrainer(ag, use_graphs=use_graphs, warmup_eager=2)
    try:
        t.run(2)
        steps = L.training_steps
        r1 = t.evaluate(n_envs=8, seed=2)
        assert r1["envs"] == 8 and r1["env_steps"] > 8 * 3 and np.isfinite(r1["return_mean"])
        assert L.training_steps == steps
        assert t.evaluate(n_envs=8, seed=2) == r1  # the same evaluator, weights and episodes
        ev = t._evaluator
        w0 = [p.detach().clone() for p in L.actor.parameters()]
        ver = [p._version for p in L.actor.parameters()]
        t.run(6)                                   # with graphs: replays from the third step on
        assert L.training_steps == steps + 6
        assert any(not torch.equal(a, b) for a, b in zip(w0, L.actor.parameters()))
        r2 = t.evaluate(n_envs=8, seed=2)
        assert t._evaluator is ev                  # kept, not rebuilt
        assert r2 != r1 and r2["return_mean"] != r1["return_mean"]
        fresh = Evaluator.from_agent(ag, 8, use_checkpoint=False, seed=2)
        try:
            assert fresh.evaluate()[0] == r2       # a new evaluator packed from the same weights
        finally:
            fresh.close()
        # the checkpoint nets are not what step() trains: still the constructor's copies
        ck = t.evaluate(n_envs=8, seed=2, use_checkpoint=True)
        assert ck != r2
        t.step()                                   # the trainer goes on
        assert L.training_steps == steps + 7
        print("version counters moved:", [p._version for p in L.actor.parameters()] != ver)
    finally:
        t.release_graphs()
    assert t._evaluator is None


def test_restart_then_reset_is_a_fresh_env():
    """VecExoskeletonEnv.restart(seed) + reset() == VecExoskeletonEnv(seed=seed).reset(),
    observations and every env's state, after an episode part that moved the
    carried state (arm pose, reference, previous actions) and the draw key."""
    from exo_amd import VecExoskeletonEnv
    n, seed = 16, 13
    kw = dict(tremor_sequence=SEQS[1], device="cuda")
    env = VecExoskeletonEnv(n, seed=seed, **kw)
    obs0 = env.reset().clone()
    st0 = [env.get_state(i) for i in (0, 7, 15)]
    acts = torch.as_tensor(np.random.default_rng(4).uniform(-1, 1, (12, n, 7)).astype(np.float32), device="cuda")
    for k in range(12):
        env.step(acts[k])
    env.reset()                                    # a second episode: its carried state differs from a fresh env's
    for k in range(5):
        env.step(acts[k])
    moved = env.reset().clone()
    assert not torch.equal(moved, obs0)
    env.restart(seed)
    obs1 = env.reset()
    assert torch.equal(obs1, obs0)
    for i, s0 in zip((0, 7, 15), st0):
        np.testing.assert_array_equal(np.asarray(env.get_state(i)), np.asarray(s0))
    outs = env.step(acts[0])
    fresh = VecExoskeletonEnv(n, seed=seed, **kw)
    assert torch.equal(fresh.reset(), obs0)
    want = fresh.step(acts[0])
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    env.restart(seed + 1)                          # another seed: other episodes
    assert not torch.equal(env.reset(), obs0)
    env.close()
    fresh.close()
