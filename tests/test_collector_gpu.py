"""exo_amd.Collector: the transitions of several noisy behaviour policies, each
on its own segment of one VecExoskeletonEnv, in a replay.LAP.

The reference is a hand-written loop on a second env with the same seed: per
step PolicySet.act with an identically initialised second MultiNoise (the
launch itself is held to each policy's own td7f_select in
tests/test_select_multi_noise_gpu.py), env.step, rows appended to host lists,
each env reset by the host after its done step (exo_reset with a mask, which
tests/test_async_episodes_gpu.py holds equal to the in-place reset).  The env
is deterministic, so the replay's rows must equal the loop's bit for bit.

Two policies on 9 and 14 envs (no multiple of 8 or 16), 240 steps: motion 0
ends after 229, so its envs are reset inside the run while the others are
still in their first episode.
"""
import functools

import numpy as np
import pytest
import torch

from test_evaluator_gpu import SEQS, _agent

pytestmark = pytest.mark.gpu

COUNTS, STEPS, SEED, TSEED = [9, 14], 240, 5, 77
SIGMA, DEC, CLIP = [0.1, 0.3], [1e-4, 0.0], [0.0, 0.5]
PER = [dict(tremor_sequence=np.array(s, dtype=np.float64)) for s in SEQS]
MOTIONS = np.concatenate([np.arange(c) % 8 for c in COUNTS])
SEG = [0, 9, 23]


def _policy_set(precision):
    from exo_amd.fused import PolicySet
    return PolicySet.from_agents([_agent(precision, 0), _agent(precision, 1)], use_checkpoint=False)


def _replay(state_dim=80):
    from exo_amd.replay import LAP
    return LAP(state_dim, 7, "cuda", num_envs=8, max_size=1024, batch_size=4)


def _env_kwargs():
    return dict(tremor_sequence=np.concatenate([np.broadcast_to(d["tremor_sequence"], (c, 7))
                                                for d, c in zip(PER, COUNTS)]))


@functools.lru_cache(maxsize=None)
def _hand_loop(precision):
    """(rows per step as host arrays, sigma at the end), computed once per precision"""
    from exo_amd import VecExoskeletonEnv
    from exo_amd.fused import MultiNoise
    ps = _policy_set(precision)
    torch.manual_seed(TSEED)  # the MultiNoise streams are keyed by torch's seed
    mn = MultiNoise(ps, SIGMA, DEC, CLIP)
    n = SEG[-1]
    env = VecExoskeletonEnv(n, motions=MOTIONS, seed=SEED, device="cuda", **_env_kwargs())
    obs = env.reset()
    outs = [env.new_outputs(False), env.new_outputs(False)]
    rows, par = [], 0
    for _ in range(STEPS):
        act = ps.act(obs, SEG, noise=mn, scale=1.0)
        nobs, rew, done, _ = env.step(act, out=outs[par], with_info=False)
        rows.append(tuple(t.cpu().numpy().copy() for t in (obs, act, nobs, rew, done)))
        if bool(done.any()):
            env.reset(mask=done, obs_out=nobs)
        obs, par = nobs, par ^ 1
    sigma = mn.sigma.cpu().numpy().copy()
    env.close()
    return rows, sigma


def _collector(precision, graph=False, replay=None, **kw):
    from exo_amd import Collector
    torch.manual_seed(TSEED)
    args = dict(sigma=SIGMA, sigma_dec=DEC, clip=CLIP, per_policy_env_kwargs=PER, seed=SEED, graph=graph)
    args.update(kw)
    return Collector(_policy_set(precision), COUNTS, replay if replay is not None else _replay(), **args)


def _expected_dataset(rows):
    """the loop's rows per stratum (motion % 8) in (step, env) order"""
    strata = MOTIONS % 8
    cols = [[] for _ in range(5)]
    sr = []
    for s in range(8):
        envs = np.flatnonzero(strata == s)
        for r in rows:
            for j in range(5):
                cols[j].append(r[j][envs])
            sr.append(np.full(len(envs), s, np.int32))
    return [np.concatenate(c) for c in cols] + [np.concatenate(sr)]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_collector_equals_the_hand_written_loop(precision, graph):
    rows, sigma = _hand_loop(precision)
    col = _collector(precision, graph)
    try:
        rep = col.collect(STEPS)
        if graph:
            assert sorted(col._graphs) == [0, 1]
        torch.cuda.synchronize()
        got = col.replay.export_dataset()
        first = col.first_return.cpu().numpy()
    finally:
        col.close()
    want = _expected_dataset(rows)
    assert len(got["reward"]) == STEPS * SEG[-1]
    for key, w in zip(("state", "action", "next_state", "reward", "done", "strata"), want):
        np.testing.assert_array_equal(got[key].numpy(), w.astype(got[key].numpy().dtype), err_msg=key)
    # resets fell inside the run, and other envs were mid-episode at its end
    done = np.stack([r[4] for r in rows]).astype(bool)
    assert done[:, MOTIONS == 0].any() and not done[:, MOTIONS != 0].any()
    # the report against the loop's lists: fp64 sums of the fp32 rewards on both sides
    rew = np.stack([r[3] for r in rows]).astype(np.float64)
    for p in range(2):
        rets = []
        for e in range(SEG[p], SEG[p + 1]):
            start = 0
            for t in np.flatnonzero(done[:, e]):
                rets.append(rew[start:t + 1, e].sum())
                start = t + 1
        r = rep[p]
        assert r["transitions"] == COUNTS[p] * STEPS and r["envs"] == COUNTS[p]
        assert r["episodes"] == len(rets) == int(done[:, SEG[p]:SEG[p + 1]].sum()) > 0
        np.testing.assert_allclose(r["return_mean"], np.mean(rets), rtol=1e-6)
        np.testing.assert_allclose(r["return_min"], np.min(rets), rtol=1e-6)
        assert np.float32(r["sigma"]) == sigma[p]
    assert np.float32(rep[0]["sigma"]) < np.float32(SIGMA[0]) and rep[1]["sigma"] == float(np.float32(SIGMA[1]))
    assert np.isnan(first[MOTIONS != 0]).all() and np.isfinite(first[MOTIONS == 0]).all()


def test_zero_sigma_first_episodes_are_the_evaluators():
    """sigma = 0: every env's first episode is the deterministic one Evaluator
    runs for the same seed and env arguments.  Compared through the returns,
    bit for bit: Collector.first_return is the fp32 sum in step order that
    Evaluator.returns is."""
    from exo_amd import Evaluator
    precision = "bf16"
    ev = Evaluator(_policy_set(precision), COUNTS, per_policy_env_kwargs=PER, seed=SEED)
    try:
        ev.evaluate()
        torch.cuda.synchronize()
        want = ev.returns.cpu().numpy().copy()
        steps = int(ev.env.lengths_host.max()) - 3
    finally:
        ev.close()
    col = _collector(precision, sigma=0.0, sigma_dec=0.0, clip=0.0)
    try:
        rep = col.collect(steps)  # the longest motion's episode: every env finishes its first
        torch.cuda.synchronize()
        got = col.first_return.cpu().numpy()
    finally:
        col.close()
    np.testing.assert_array_equal(got, want)
    assert all(r["episodes"] >= r["envs"] for r in rep)


def test_collected_dataset_trains_offline(tmp_path):
    from exo_amd import OfflineTrainer
    from exo_amd.td7 import Agent, Hyperparameters

    def agent():
        torch.manual_seed(31)
        return Agent(80, 7, 1, offline=True, hp=Hyperparameters(batch_size=5, target_update_rate=4), env_num=8,
                     buffer_size=1024, precision="bf16", graph_safe=True)
    from exo_amd import Collector
    ag = agent()
    # the behaviour policies: two agents' checkpoint nets
    col = Collector.from_agents([_agent("bf16", 0), _agent("bf16", 1)], ag.replay_buffer, envs_per_policy=COUNTS,
                                sigma=SIGMA, sigma_dec=DEC, clip=CLIP, per_policy_env_kwargs=PER, seed=SEED)
    assert col.max_action == 1.0 and len(col.policy_set) == 2
    try:
        rep = col.collect(40)
    finally:
        col.close()
    assert sum(r["transitions"] for r in rep) == 40 * SEG[-1] == int(ag.replay_buffer.size_s.sum())
    path = tmp_path / "dataset.pt"
    ag.save_dataset(path)
    fresh = agent()
    fresh.load_dataset(path)
    assert int(fresh.replay_buffer.size_s.sum()) == 40 * SEG[-1]
    tr = OfflineTrainer(fresh, use_graphs=False)
    for _ in range(4):
        tr.step()
    torch.cuda.synchronize()
    L = fresh.learner
    for net in (L.actor, L.critic, L.encoder):
        assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    assert bool(torch.isfinite(fresh.replay_buffer.priority).all())


def test_argument_errors_launch_nothing():
    rb = _replay()
    with pytest.raises(ValueError, match="sigma"):
        _collector("bf16", replay=rb, sigma=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="sigma"):
        _collector("bf16", replay=rb, sigma=[0.1, -0.2])
    with pytest.raises(ValueError, match="physics"):
        _collector("bf16", replay=rb, physics="rigid")
    with pytest.raises(ValueError, match="dimensional"):
        _collector("bf16", replay=_replay(40))
    with pytest.raises(ValueError, match="per_policy_env_kwargs"):
        _collector("bf16", replay=rb, per_policy_env_kwargs=PER[:1])
    with pytest.raises(ValueError, match="strata"):
        _collector("bf16", replay=rb, strata=np.zeros(5, np.int32))
    from exo_amd import Collector
    with pytest.raises(ValueError, match="envs_per_policy"):
        Collector(_policy_set("bf16"), [9], rb)
    col = _collector("bf16", replay=rb, sigma_dec=[1e-3, 0.0])  # 0.1 lasts 100 steps
    try:
        with pytest.raises(ValueError, match="below 0"):
            col.collect(101)
        torch.cuda.synchronize()
        assert int(rb.size_s.sum()) == 0 and col.noise.counters() == [0, 0] and col.steps_run == 0
        col.collect(3)
        assert int(rb.size_s.sum()) == 3 * SEG[-1] and col.noise.counters() == [3, 3]
        with pytest.raises(ValueError, match="below 0"):
            col.collect(98)
    finally:
        col.close()
