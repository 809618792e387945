"""td7f_select_seq / FusedNets.select(pink=PinkNoise.for_learner(...)) on the
MI355X: the learner's own select launch (its packed weights, 16- or 32-row
tiles, workgroup cap, zs / actor split) with each env's own column of its
coloured noise sequence (TD7_multi_agent_Pink_noise.py:203-228 per env).

The kernel runs select_kernel's rows and adds a term it only loads, so its
output equals the multi-policy launch with one policy (same body) and the
deterministic launch followed by the same three fp32 operations in torch, bit
for bit.  Policy, observations: test_select_multi_gpu.py's."""
import ctypes

import numpy as np
import pytest
import torch

from test_select_multi_gpu import _agent, _bits, _obs, _policy_set

pytestmark = pytest.mark.gpu

N = 38  # three 16-row tiles or two 32-row tiles, the last one ragged either way
SIGMA, DEC, CLIP, SCALE = 0.2, 1e-3, 0.15, 0.75


def _lengths(n):
    ln = np.random.default_rng(4).choice([232, 347, 288, 17], size=n)
    ln[:3] = (347, 17, 232)
    return ln


def _setup(precision):
    """(agent, its PinkNoise, obs, t): sigma, decay and clip as above, mixed step
    indices -- the first step, the last column of a row, and in between"""
    from exo_amd.fused import PinkNoise
    ag = _agent(precision, "default", 0)
    L = ag.learner
    L.exploration_noise_t.fill_(SIGMA)
    L.action_noise_decrease = DEC
    ln = _lengths(N)
    pn = PinkNoise.for_learner(L.fused, ln, clip=CLIP)
    t = np.random.default_rng(6).integers(0, ln)
    t[0], t[1], t[5], t[37] = 0, ln[1] - 1, ln[5] - 1, ln[37] - 1
    pn.t.copy_(torch.as_tensor(t.astype(np.int32)))
    return ag, pn, _obs(N), t


def _deterministic(ag, obs, rt):
    """the agent's own td7f_select at sigma 0, scale 1; the noise state restored"""
    L = ag.learner
    sig, rng = L.exploration_noise_t.clone(), L._explore_rng.state.clone()
    L.exploration_noise_t.fill_(0.0)
    a = L.fused.select(obs, rt=rt).clone()
    torch.cuda.synchronize()
    L.exploration_noise_t.copy_(sig)
    L._explore_rng.state.copy_(rng)
    return a


def _noise_terms(pn, t):
    e = pn.seq[torch.arange(pn.n, device="cuda"), torch.as_tensor(t, device="cuda")]
    return e, e.clamp(-CLIP, CLIP)


def _want(ag, pn, obs, t, rt):
    e, ec = _noise_terms(pn, t)
    return torch.clamp(_deterministic(ag, obs, rt) + ec, -1.0, 1.0) * SCALE, e


def _raw(ag, pn, obs, out, rt=0, wg_cap=0, mode=0, zimg=None):
    """td7f_select_seq as it stands in the C ABI, into `out`"""
    from exo_amd import _native as nat
    from exo_amd.fused import _lin_array
    fz = ag.learner.fused
    fz.refresh("fixed_encoder", "actor")
    nz = pn.noise(SCALE)
    fe = fz.nets["fixed_encoder"].layers
    return nat.lib().td7f_select_seq(fz.prec, fz.act, _lin_array(fe[:3]), fz.nets["actor"].array, nat.ptr(obs),
                                     obs.shape[0], ctypes.byref(nz), nat.ptr(pn.seq), nat.ptr(pn.t), pn.Lmax,
                                     nat.ptr(out), wg_cap, rt, nat.ptr(zimg), mode, nat.stream_ptr(obs.device))


def _assert_nonvacuous(pn, t):
    e, _ = _noise_terms(pn, t)
    assert bool((e.abs() > 0).any(1).all())  # every row has a noise term
    assert bool((pn.seq.abs().amax((1, 2)) > CLIP).all())  # and the clip has something to cut in every row


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_equals_the_multi_policy_launch_with_one_policy(precision):
    from exo_amd.fused import PinkNoise
    ag, pn, obs, t = _setup(precision)
    _assert_nonvacuous(pn, t)
    # td7f_select_multi_seq, K = 1, seg = [0, N]: the same weights, table and t
    ps = _policy_set([ag])
    pm = PinkNoise(ps, [0, N], _lengths(N), SIGMA, DEC, CLIP)
    assert pm.Lmax == pn.Lmax
    pm.seq.copy_(pn.seq)
    pm.t.copy_(pn.t)
    want = ps.act(obs, [0, N], scale=SCALE, noise=pm).clone()
    G = 16
    guard = torch.full((N + 2 * G, 7), float("nan"), device="cuda")
    out = guard[G:G + N]
    assert _raw(ag, pn, obs, out, rt=1) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    assert bool(torch.isnan(guard[:G]).all()) and bool(torch.isnan(guard[G + N:]).all())
    # ... and it is the host wrapper's launch; a second call without advance adds the same terms
    for _ in range(2):
        got = ag.learner.fused.select(obs, scale=SCALE, rt=1, pink=pn)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(want))
    assert not torch.equal(_bits(want), _bits(_deterministic(ag, obs, 1) * SCALE))


def test_32_row_tiles_equal_the_deterministic_launch_plus_the_column():
    ag, pn, obs, t = _setup("bf16")
    _assert_nonvacuous(pn, t)
    want, _ = _want(ag, pn, obs, t, 2)
    got = ag.learner.fused.select(obs, scale=SCALE, rt=2, pink=pn)
    torch.cuda.synchronize()
    assert torch.equal(got, want)  # by value: a + 0 in the reference launch may have lost a zero's sign
    assert not bool(torch.isnan(got).any())


def test_workgroup_cap_two_launches_one_decrement():
    ag, pn, obs, t = _setup("bf16")
    L = ag.learner
    one = torch.empty((N, 7), device="cuda")
    assert _raw(ag, pn, obs, one, rt=1) == 0
    torch.cuda.synchronize()
    sigma0 = L.exploration_noise_t.clone()
    states0 = [pn.rngs[0].state.clone(), L._explore_rng.state.clone()]
    seq0, t0 = pn.seq.clone(), pn.t.clone()
    two = torch.empty((N, 7), device="cuda")
    assert _raw(ag, pn, obs, two, rt=1, wg_cap=2) == 0  # 3 tiles: launches of 2 and 1 workgroups
    torch.cuda.synchronize()
    assert torch.equal(_bits(two), _bits(one))
    want_sigma = np.float32(sigma0.item()) - np.float32(DEC)
    assert np.float32(L.exploration_noise_t.item()) == want_sigma and want_sigma < np.float32(sigma0.item())
    assert int(pn.ticket[0]) == 0
    assert torch.equal(pn.rngs[0].state, states0[0]) and torch.equal(L._explore_rng.state, states0[1])
    assert torch.equal(_bits(pn.seq), _bits(seq0)) and torch.equal(pn.t, t0)


@pytest.mark.parametrize("precision,rt", [("fp32", None), ("bf16", 2)])
def test_zs_half_then_actor_half_equals_one_launch(precision, rt):
    ag, pn, obs, t = _setup(precision)
    fz = ag.learner.fused
    whole = fz.select(obs, scale=SCALE, rt=rt, pink=pn).clone()
    sigma1 = ag.learner.exploration_noise_t.clone()
    img = fz.select_zs(obs, rt=rt)
    torch.cuda.synchronize()
    assert torch.equal(ag.learner.exploration_noise_t, sigma1)  # the zs half touches no noise state
    halves = fz.select(obs, scale=SCALE, rt=rt, zs_img=img, pink=pn)
    torch.cuda.synchronize()
    assert torch.equal(_bits(halves), _bits(whole))
    assert np.float32(ag.learner.exploration_noise_t.item()) == np.float32(sigma1.item()) - np.float32(DEC)


def test_step_index_is_clamped_to_the_table():
    ag, pn, obs, t = _setup("bf16")
    pn.t[3] = pn.Lmax + 5
    pn.t[4] = -2
    t = t.copy()
    t[3], t[4] = pn.Lmax - 1, 0
    want, _ = _want(ag, pn, obs, t, 1)
    got = ag.learner.fused.select(obs, scale=SCALE, rt=1, pink=pn)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_select_action_batch_routes_and_refuses():
    ag, pn, obs, t = _setup("bf16")
    want = ag.learner.fused.select(obs, scale=ag.max_action, pink=pn).clone()
    got = ag.select_action_batch(obs, pink=pn)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want))
    with pytest.raises(ValueError):
        ag.select_action_batch(obs, pink=pn, use_checkpoint=True)
    with pytest.raises(ValueError):
        ag.learner.fused.select(_obs(N - 1), pink=pn)  # built for N envs
