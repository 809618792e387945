"""exo_amd.Collector(noise="pink"): datasets collected with one coloured noise
sequence per env (fused.PinkNoise), regenerated on the device when the env's
episode ends.

Three policies on 5, 0 and 33 envs, 400 steps: the longest motion ends after
346, so every env passes at least one reset and draws a second sequence.  The
reference is a hand-written loop over the same PinkNoise calls on a second env
with the same seed, each finished env reset by the host (exo_reset with a
mask, which tests/test_async_episodes_gpu.py holds equal to the in-place
reset); the env is deterministic, so the datasets are equal bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

from test_evaluator_gpu import _agent

pytestmark = pytest.mark.gpu

COUNTS, STEPS, SEED, TSEED = [5, 0, 33], 400, 5, 77
SEG = [0, 5, 5, 38]
SIGMA, DEC, CLIP = [0.1, 0.2, 0.3], [1e-4, 1e-4, 0.0], [0.0, 0.0, 0.25]
MOTIONS = np.concatenate([np.arange(c) % 8 for c in COUNTS])
KEYS = ("state", "action", "next_state", "reward", "done", "strata")


def _policy_set():
    from exo_amd.fused import PolicySet
    return PolicySet.from_agents([_agent("bf16", k) for k in range(3)], use_checkpoint=False)


def _replay():
    from exo_amd.replay import LAP
    return LAP(80, 7, "cuda", num_envs=8, max_size=4096, batch_size=4)


def _collector(graph=False, **kw):
    from exo_amd import Collector
    ps = _policy_set()  # (building an agent for the first time seeds torch)
    torch.manual_seed(TSEED)  # the noise streams are keyed by torch's seed
    args = dict(sigma=SIGMA, sigma_dec=DEC, clip=CLIP, seed=SEED, graph=graph, noise="pink")
    args.update(kw)
    return Collector(ps, COUNTS, _replay(), **args)


@functools.lru_cache(maxsize=None)
def _collected(graph):
    """(dataset as numpy arrays, report, first returns, episode indices) of one 400-step run"""
    col = _collector(graph)
    try:
        rep = col.collect(STEPS)
        if graph:
            assert sorted(col._graphs) == [0, 1]
        torch.cuda.synchronize()
        data = {k: v.numpy().copy() for k, v in col.replay.export_dataset().items() if k in KEYS}
        return data, rep, col.first_return.cpu().numpy(), col.noise.epi.cpu().numpy()
    finally:
        col.close()


def test_graph_replay_equals_eager_steps():
    eager, rep_e, first_e, epi_e = _collected(False)
    graph, rep_g, first_g, epi_g = _collected(True)
    assert len(eager["reward"]) == STEPS * SEG[-1]
    for k in KEYS:
        np.testing.assert_array_equal(eager[k].view(np.uint8), graph[k].view(np.uint8), err_msg=k)
    np.testing.assert_equal(rep_e, rep_g)  # (the policy without envs reports NaN returns)
    np.testing.assert_array_equal(first_e.view(np.int32), first_g.view(np.int32))
    # every env finished an episode and drew a new sequence
    assert (epi_e >= 1).all() and np.array_equal(epi_e, epi_g)
    assert np.isfinite(first_e).all()
    assert [r["episodes"] > 0 for r in rep_e] == [True, False, True]
    # 400 fp32 subtractions of the decay, each rounded at magnitude <= 0.1
    assert abs(rep_e[0]["sigma"] - (SIGMA[0] - STEPS * DEC[0])) <= STEPS * 2.0 ** -24 * SIGMA[0]
    assert rep_e[1]["sigma"] == float(np.float32(SIGMA[1]))  # no envs: its sigma never moves


def test_collector_equals_the_hand_written_loop():
    from exo_amd import VecExoskeletonEnv
    from exo_amd.fused import PinkNoise
    got = _collected(False)[0]
    ps = _policy_set()
    n = SEG[-1]
    env = VecExoskeletonEnv(n, motions=MOTIONS, seed=SEED, device="cuda")
    torch.manual_seed(TSEED)
    pn = PinkNoise(ps, SEG, env.lengths_host, SIGMA, DEC, CLIP)
    ones = torch.ones(n, dtype=torch.bool, device="cuda")
    obs = env.reset()
    outs = [env.new_outputs(False), env.new_outputs(False)]
    rows, par = [], 0
    for _ in range(STEPS):
        act = ps.act(obs, SEG, noise=pn, scale=1.0)
        nobs, rew, done, _ = env.step(act, out=outs[par], with_info=False)
        rows.append(tuple(t.cpu().numpy().copy() for t in (obs, act, nobs, rew, done)))
        pn.advance(ones, done)
        if bool(done.any()):
            env.reset(mask=done, obs_out=nobs)
        obs, par = nobs, par ^ 1
    env.close()
    # the loop's rows per stratum (motion % 8) in (step, env) order
    strata = MOTIONS % 8
    cols = [[] for _ in range(6)]
    for s in range(8):
        envs = np.flatnonzero(strata == s)
        for r in rows:
            for j in range(5):
                cols[j].append(r[j][envs])
            cols[5].append(np.full(len(envs), s, np.int32))
    for key, c in zip(KEYS, cols):
        w = np.concatenate(c).astype(got[key].dtype)
        np.testing.assert_array_equal(got[key].view(np.uint8), w.view(np.uint8), err_msg=key)
    # the noise was there, and it is not the Gaussian collector's
    acts = np.stack([r[1] for r in rows])
    det = ps.act(torch.as_tensor(rows[0][0], device="cuda"), SEG).cpu().numpy()
    assert not np.array_equal(acts[0], det)


def test_zero_sigma_first_returns_equal_the_gaussian_collectors():
    res = []
    for kind in ("pink", "gaussian"):
        col = _collector(noise=kind, sigma=0.0, sigma_dec=0.0, clip=0.0)
        try:
            col.collect(STEPS)
            torch.cuda.synchronize()
            res.append(col.first_return.cpu().numpy())
        finally:
            col.close()
    assert np.isfinite(res[0]).all()
    np.testing.assert_array_equal(res[0].view(np.int32), res[1].view(np.int32))


def test_unknown_noise_is_refused():
    from exo_amd import Collector
    with pytest.raises(ValueError, match="noise"):
        Collector(_policy_set(), COUNTS, _replay(), noise="nonsense")
