"""td7f_select_multi / exo_amd.fused.PolicySet on the MI355X: several policies
act in one launch, policy p on the rows [seg[p], seg[p+1]) of the observations.

The kernel runs select_kernel's per-row arithmetic (16-row tiles) from the same
building blocks, and that arithmetic does not depend on a row's slot in its
tile (MFMA rows are independent, norm_fwd reduces within a row), so against
the single-policy launch td7f_select (rt = 1) the comparisons are bit for bit:
with the exploration noise for K = 1, and deterministically (sigma = 0 around
the reference call) for ragged segments whose starts are off the 16-row grid.
The golden parity runs the checkpoint nets through a fused kernel for the
first time, at test_select_full_gpu.py's bounds.

Shapes: the default widths (5 weight tiles per wave, TH 5) and all-256 (TH 4).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import GOLDEN, SELECT_FULL, select_full_perturb, select_full_states
from test_select_full_gpu import _agent as _golden_agent, _emulate_bf16, _perturb_on_device

pytestmark = pytest.mark.gpu

SHAPES = {"default": {}, "w256": dict(zs_dim=256, enc_hdim=256, critic_hdim=256, actor_hdim=256)}


@functools.lru_cache(maxsize=None)
def _agent(precision, shape, k):
    """Agent k of (precision, shape): seeded init, live actor / fixed encoder
    perturbed (select_full_perturb), so no two agents -- and no agent's live
    and checkpoint nets -- share weights."""
    from exo_amd.td7 import Agent, Hyperparameters
    torch.manual_seed(300 + k)
    ag = Agent(80, 7, 1, hp=Hyperparameters(**SHAPES[shape]), env_num=8, device="cuda", buffer_size=64,
               precision=precision)
    assert ag.learner.fused is not None
    _perturb_on_device(ag.learner.actor, 7000 + 100 * k, select_full_perturb)
    _perturb_on_device(ag.learner.fixed_encoder, 7050 + 100 * k, select_full_perturb)
    return ag


@functools.lru_cache(maxsize=None)
def _obs(n):
    st = select_full_states()
    assert n <= len(st)
    return torch.as_tensor(st[:n], device="cuda")


def _policy_set(agents, live=True):
    from exo_amd.fused import PolicySet
    return PolicySet.from_agents(agents, use_checkpoint=not live)


def _noise_state(L):
    return L.exploration_noise_t.clone(), L._explore_rng.state.clone()


def _deterministic_single(ag, obs):
    """the agent's own td7f_select (16-row tiles) with sigma = 0; the noise state restored"""
    L = ag.learner
    sig, rng = _noise_state(L)
    L.exploration_noise_t.fill_(0.0)
    a = L.fused.select(obs, rt=1).clone()
    torch.cuda.synchronize()
    L.exploration_noise_t.copy_(sig)
    L._explore_rng.state.copy_(rng)
    return a


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", ["default", "w256"])
@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
def test_one_policy_equals_select_with_noise(precision, shape):
    ag = _agent(precision, shape, 0)
    L, fz = ag.learner, ag.learner.fused
    n = 37  # two full tiles + 5 rows
    obs = _obs(n)
    ps = _policy_set([ag])
    sig0, rng0 = _noise_state(L)
    want = fz.select(obs, rt=1).clone()
    torch.cuda.synchronize()
    sig1, rng1 = _noise_state(L)
    assert not torch.equal(sig0, sig1) and not torch.equal(rng0, rng1)  # the launch drew and advanced
    L.exploration_noise_t.copy_(sig0)
    L._explore_rng.state.copy_(rng0)
    nz = fz._noise(L._explore_rng, L.exploration_noise_t, L.action_noise_decrease * n, 0.0, 1.0)
    got = ps.act(obs, [0, n], noise=nz)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want))
    sig2, rng2 = _noise_state(L)
    assert torch.equal(_bits(sig2), _bits(sig1)) and torch.equal(rng2, rng1)  # sigma, call counter, ticket
    # and the noise was there: the deterministic launch differs
    assert not torch.equal(_bits(ps.act(obs, [0, n])), _bits(want))


@pytest.mark.parametrize("shape", ["default", "w256"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_ragged_segments_deterministic(precision, shape):
    from exo_amd import _native as nat
    agents = [_agent(precision, shape, k) for k in range(4)]
    seg = [0, 5, 5, 40, 57]  # lengths 5, 0, 35, 17: starts off the 16-row grid
    n, scale, G = seg[-1], 0.75, 16
    obs = _obs(n)
    ps = _policy_set(agents)
    # the C tile plan is the numpy one
    from exo_amd.fused import multi_tiles
    cseg = (ctypes.c_int32 * 5)(*seg)
    buf = (ctypes.c_int32 * (3 * 16))()
    nt = nat.lib().td7f_multi_tiles(4, cseg, buf, 16)
    assert nt == 6 and nat.lib().td7f_multi_tiles(4, cseg, None, 0) == 6
    np.testing.assert_array_equal(np.ctypeslib.as_array(buf)[:18].reshape(6, 3), multi_tiles(seg))
    before = [_noise_state(a.learner) for a in agents]
    guard = torch.full((n + 2 * G, 7), float("nan"), device="cuda")
    out = guard[G:G + n]
    ps.act(obs, seg, out=out, scale=scale)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    assert bool(torch.isnan(guard[:G]).all()) and bool(torch.isnan(guard[G + n:]).all())
    for a, (sig, rng) in zip(agents, before):  # noise=None reads and writes no noise state
        assert torch.equal(_bits(a.learner.exploration_noise_t), _bits(sig))
        assert torch.equal(a.learner._explore_rng.state, rng)
    for p, ag in enumerate(agents):
        a, b = seg[p], seg[p + 1]
        if b == a:
            continue
        want = _deterministic_single(ag, obs)[a:b] * scale
        assert torch.equal(_bits(out[a:b]), _bits(want)), f"segment {p}"
    # the segments really are different policies
    assert not torch.equal(out[0:5], _deterministic_single(agents[2], obs)[0:5] * scale)


@pytest.mark.parametrize("case", [0, 1])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_golden_checkpoint_and_live(precision, case):
    from exo_amd.fused import PolicySet
    g = np.load(f"{GOLDEN}/select_action_full.npz", allow_pickle=False)
    name, kw, seed = SELECT_FULL[case]
    ag = _golden_agent(name, kw, seed, precision)
    L = ag.learner
    st = g["state"]
    assert len(st) == 256
    ps = PolicySet([(L.checkpoint_actor, L.checkpoint_encoder), (L.actor, L.fixed_encoder)], precision, "cuda",
                   activations=(ag.hp.enc_activ, ag.hp.actor_activ))
    obs = torch.as_tensor(np.concatenate([st, st]), device="cuda")
    out = ps.act(obs, [0, 256, 512]).cpu().numpy()
    for p, (ckpt, key) in enumerate(((True, "ckpt"), (False, "live"))):
        got, want = out[256 * p:256 * (p + 1)], g[f"{name}.{key}"]
        e_ref = float(np.abs(got - want).max())
        if precision == "fp32":
            print(name, key, f"|gpu - ref| {e_ref:.3g}")
            assert e_ref <= 2e-5, f"{name}.{key}: |gpu - ref| {e_ref:.3g}"
            continue
        emu = _emulate_bf16(ag, st, ckpt)
        e_emu, e_to_emu = float(np.abs(emu - want).max()), float(np.abs(got - emu).max())
        print(name, key, f"|gpu - ref| {e_ref:.3g} |gpu - emu| {e_to_emu:.3g} |emu - ref| {e_emu:.3g}")
        assert e_ref <= 1.5 * e_emu + 5e-4, f"{name}.{key}: |gpu - ref| {e_ref:.3g} (emulation {e_emu:.3g})"
        assert e_to_emu <= 2e-3, f"{name}.{key}: |gpu - bf16 emulation| {e_to_emu:.3g}"


def test_argument_errors_launch_nothing():
    from exo_amd import _native as nat
    from exo_amd.fused import TD7FLin, select_multi_raw
    EINVAL = -22
    a, b = _agent("bf16", "default", 0), _agent("bf16", "default", 1)
    c = _agent("bf16", "w256", 0)
    ps, psc = _policy_set([a, b]), _policy_set([c])
    n = 40
    seg = [0, 24, 40]
    obs = _obs(n)
    key, tiles, nt = ps.tiles(seg)
    out = torch.full((n, 7), 7.0, device="cuda")

    def call(enc=ps.enc, actor=ps.actor, seg=seg, n=n, npol=2, nt=nt):
        rc = select_multi_raw(ps.prec, ps.act_codes, enc, actor, ps.table, seg, tiles, nt, obs, n, None, out, 1.0,
                              npol=npol)
        torch.cuda.synchronize()
        return rc

    def mixed(x, y, per):  # policy 0 of x, policy 0 of y
        return (TD7FLin * (2 * per))(*(list(x)[:per] + list(y)[:per]))
    assert call(enc=mixed(ps.enc, psc.enc, 3), actor=mixed(ps.actor, psc.actor, 4)) == EINVAL  # other widths
    assert call(actor=mixed(ps.actor, psc.actor, 4)) == EINVAL
    assert call(seg=[0, 41, 40]) == EINVAL          # decreasing
    assert call(seg=[0, 24, 39]) == EINVAL          # seg[K] != n
    assert call(seg=[1, 24, 40]) == EINVAL          # seg[0] != 0
    assert call(npol=0) == EINVAL
    assert call(nt=nt + 1) == EINVAL                # a tile table of another seg
    assert bool((out == 7.0).all())
    nat.lib().td7f_probe(1)
    try:
        assert call() == 0                          # plan-only: valid, nothing launched
    finally:
        nat.lib().td7f_probe(0)
    assert bool((out == 7.0).all())
    assert call() == 0
    assert bool((out != 7.0).all())
    # the host side refuses mixed shapes before any launch
    from exo_amd.fused import PolicySet
    with pytest.raises(ValueError, match="shape"):
        PolicySet.from_agents([a, c], use_checkpoint=False)
    with pytest.raises(ValueError, match="entries"):
        ps.act(obs, [0, 40])


def test_refresh_repacks_the_changed_policy():
    a, b = _agent("bf16", "default", 2), _agent("bf16", "default", 3)
    seg = [0, 21, 50]
    obs = _obs(50)
    ps = _policy_set([a, b])
    first = ps.act(obs, seg).clone()
    w = b.learner.actor.l2.weight
    saved = w.detach().clone()
    try:
        with torch.no_grad():
            w.mul_(1.5)
        stale = ps.act(obs, seg).clone()
        assert torch.equal(_bits(stale), _bits(first))  # packed copies: nothing moves before refresh()
        ps.refresh()
        got = ps.act(obs, seg)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got[:21]), _bits(first[:21]))
        assert not torch.equal(_bits(got[21:]), _bits(first[21:]))
        assert torch.equal(_bits(got[21:]), _bits(_deterministic_single(b, obs)[21:]))
    finally:
        with torch.no_grad():
            w.copy_(saved)


def test_new_seg_inside_a_capture_raises():
    a = _agent("bf16", "default", 0)
    ps = _policy_set([a])
    obs = _obs(20)
    out = torch.empty((20, 7), device="cuda")
    ps.act(obs, [0, 20], out=out)
    ps._tiles.clear()
    real = torch.cuda.is_current_stream_capturing
    torch.cuda.is_current_stream_capturing = lambda: True  # no capture needed to see the refusal
    try:
        with pytest.raises(RuntimeError, match="before graph capture"):
            ps.act(obs, [0, 20], out=out)
    finally:
        torch.cuda.is_current_stream_capturing = real
