"""VecTrainer(episodes="async", exploration="pink_env"): coloured exploration
noise with one sequence per env and episode (TD7_multi_agent_Pink_noise.py
:203-228 per env) inside the graph-replayed loop -- td7f_select_seq in place of
the Gaussian select, one td7f_pink_advance launch after the env step.

Shapes: test_async_episodes_gpu._trainer's 64 envs (8 per motion), batch 16,
env_num 8, graph_safe -- but 256-wide nets, not its 32-wide ones: "pink_env"
needs the fused select launch, and the fused passes take hidden widths of
193..320 only (exo_amd.fused.supported); 32-wide learners have no fused path,
so the trainer refuses them.  256 is the width the other fused trainer tests
use (test_rollout_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, ITERS, FIRST_END = 64, 240, 229  # motion 0 (232 samples) ends its first episode at iteration 229
SEED = 3


def _trainer(precision="bf16", budget=0, use_graphs=True, **kw):
    from exo_amd import VecExoskeletonEnv
    from exo_amd.rollout import VecTrainer
    from exo_amd.td7 import Agent, Hyperparameters
    torch.manual_seed(SEED)
    hp = Hyperparameters(zs_dim=256, enc_hdim=256, critic_hdim=256, actor_hdim=256, batch_size=16,
                         target_update_rate=50)
    env = VecExoskeletonEnv(N, seed=SEED)
    if budget:
        env.set_step_budget(budget)
    agent = Agent(80, 7, 1, hp=hp, env_num=8, buffer_size=8192, graph_safe=True, precision=precision)
    assert agent.learner.fused is not None
    kw.setdefault("episodes", "async")
    kw.setdefault("exploration", "pink_env")
    return VecTrainer(env, agent, use_graphs=use_graphs, **kw), env, agent


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _run(precision, use_graphs):
    """240 iterations, no step budget; what the tests compare, as clones"""
    tr, env, ag = _trainer(precision, use_graphs=use_graphs)
    pn = tr.pink
    L = ag.learner
    res = dict(fill=pn.seq.clone(), sigma0=np.float32(L.exploration_noise_t.item()),
               dec=np.float32(L.action_noise_decrease), lengths=np.array(env.lengths_host), Lmax=pn.Lmax)
    assert int(pn.t.abs().sum()) == 0 and int(pn.epi.abs().sum()) == 0  # the first fill is episode 0, step 0
    if use_graphs:
        tr.plan(ITERS)  # the overlapped pairs run only inside an announced run
    for _ in range(ITERS):
        assert tr.step() == N
    torch.cuda.synchronize()
    res.update(actor=[p.detach().clone() for p in L.actor.parameters()], obs=tr.obs.clone(), seq=pn.seq.clone(),
               t=pn.t.clone(), epi=pn.epi.clone(), sigma=L.exploration_noise_t.clone(),
               total=tr.env_steps_total(), resets=tr.resets, graphs=list(tr.graphs),
               counts=np.array([env.get_state(e)[0] for e in range(N)]), fused=L.fused, motions=np.array(env.motions))
    return res


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_graph_replay_equals_eager(precision):
    """Graph-replayed (overlapped pairs; fp32: the split select, whose actor
    half is td7f_select_seq's mode 2) against eager, same seeds: bit-equal."""
    g, e = _run(precision, True), _run(precision, False)
    assert any(k[-1] == "overlap" for k in g["graphs"]) and not e["graphs"]
    m0 = g["motions"] == 0
    np.testing.assert_array_equal(g["lengths"][m0], FIRST_END + 3)
    assert bool((g["epi"].cpu().numpy()[m0] == 1).all())  # motion 0's envs did end their first episode
    for a, b in zip(g["actor"], e["actor"]):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(g["obs"]), _bits(e["obs"]))
    assert torch.equal(_bits(g["seq"]), _bits(e["seq"]))
    assert torch.equal(g["t"], e["t"]) and torch.equal(g["epi"], e["epi"])
    assert torch.equal(_bits(g["sigma"]), _bits(e["sigma"]))
    assert g["total"] == e["total"] == N * ITERS and g["resets"] == 0


def _sigma_after(res, calls):
    """the schedule on the host in fp32: one decrement per select call (:225)"""
    s = res["sigma0"]
    for _ in range(calls):
        s = np.float32(s - res["dec"])
    return s


def test_state_machine_and_regenerated_rows():
    res = _run("bf16", True)
    m0 = res["motions"] == 0
    t, epi = res["t"].cpu().numpy(), res["epi"].cpu().numpy()
    np.testing.assert_array_equal(epi[m0], 1)
    np.testing.assert_array_equal(t[m0], ITERS - FIRST_END)  # 11 actions into the second episode
    np.testing.assert_array_equal(epi[~m0], 0)
    np.testing.assert_array_equal(t[~m0], ITERS)
    np.testing.assert_array_equal(t, res["counts"] - 2)  # the env's own step counter (2 at a reset)
    assert np.float32(res["sigma"].item()) == _sigma_after(res, ITERS)
    fill, seq = res["fill"], res["seq"]
    keep = torch.as_tensor(~m0, device="cuda")
    assert torch.equal(_bits(seq[keep]), _bits(fill[keep]))  # rows of envs that did not reset: untouched
    new = torch.as_tensor(m0, device="cuda")
    assert bool((seq[new] != fill[new]).flatten(1).any(1).all())  # every reset env has a new sequence
    # the regenerated rows against a stand-alone PinkNoise of the same stream
    # (tag, seed), its sigma bound to a tensor of this test: the fill, then one
    # advance with motion 0's envs flagged at the sigma of iteration 229 --
    # that iteration's select has decremented it before the advance reads it
    from exo_amd.fused import PinkNoise
    torch.manual_seed(SEED)  # DeviceRNG keys follow torch.initial_seed()
    sig = torch.full((), float(res["sigma0"]), dtype=torch.float32, device="cuda")
    ref = PinkNoise.for_learner(res["fused"], res["lengths"], sigma=sig)
    assert torch.equal(_bits(ref.seq), _bits(fill))
    sig.fill_(float(_sigma_after(res, FIRST_END)))
    ref.advance(torch.ones(N, dtype=torch.bool, device="cuda"), new)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ref.seq[new]), _bits(seq[new]))
    peak = seq[new].abs().amax((1, 2)).cpu().numpy()
    np.testing.assert_allclose(peak, _sigma_after(res, FIRST_END), rtol=1e-6)  # peak-normalised, times that sigma


def test_step_budget():
    """Budget 4: solves span launches, envs skip launches, and an env is reset
    launches after its `done` step: t and epi still follow each env's own
    episode (the env's step counter and the resets seen from the host)."""
    tr, env, ag = _trainer("bf16", budget=4)
    pn = tr.pink
    m0 = np.array(env.motions) == 0
    finished = np.zeros(N, np.int64)
    prev = np.full(N, 2)
    stepped_sum, it = 0, 0
    while not (finished[m0] >= 1).all():
        assert tr.step() == 0
        it += 1
        stepped_sum += int(tr._pink_stepped.sum())
        assert it < FIRST_END * 64, "does not converge"
        if it % 5 == 0:
            counts = np.array([env.get_state(e)[0] for e in range(N)])
            finished += counts < prev  # an episode is hundreds of steps: at most one reset between looks
            prev = counts
            np.testing.assert_array_equal(pn.t.cpu().numpy(), counts - 2)
            np.testing.assert_array_equal(pn.epi.cpu().numpy(), finished)
    assert tr.env_steps_total() == stepped_sum
    assert stepped_sum < N * it  # launches were skipped: the masks mattered
    assert it > FIRST_END and tr.resets == 0
    fill_changed = (pn.epi > 0).cpu().numpy()
    np.testing.assert_array_equal(fill_changed, finished > 0)


def test_refusals():
    with pytest.raises(ValueError):
        _trainer(episodes="sync")
    with pytest.raises(ValueError):  # as before: "pink" indexes its noise by the round's step
        _trainer(exploration="pink")
    from exo_amd import VecExoskeletonEnv
    from exo_amd.rollout import VecTrainer
    from exo_amd.td7 import Agent, Hyperparameters
    hp = Hyperparameters(zs_dim=32, enc_hdim=32, critic_hdim=32, actor_hdim=32, batch_size=16)
    agent = Agent(80, 7, 1, hp=hp, env_num=8, buffer_size=1024)
    assert agent.learner.fused is None
    with pytest.raises(ValueError):  # no fused select launch at these widths
        VecTrainer(VecExoskeletonEnv(16, seed=1), agent, episodes="async", exploration="pink_env")
