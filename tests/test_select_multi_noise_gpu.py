"""td7f_select_multi_noise / exo_amd.fused.MultiNoise on the MI355X: several
policies act in one launch, each with its own exploration-noise state (sigma,
clip, decay, Philox stream).

The kernel runs select_multi_kernel's rows and noise_rows' arithmetic with a
segment-local Philox element, so policy p's rows equal policy p's own
td7f_select (rt = 1) on them -- noise, sigma and call counter included -- bit
for bit, whichever policies share the launch and wherever the segment starts.
Given normals are checked against the closed form in fp64.

Agents, observations and shapes are test_select_multi_gpu.py's.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_select_multi_gpu import _agent, _bits, _obs, _policy_set

pytestmark = pytest.mark.gpu

SEG = [0, 5, 5, 40, 57]  # lengths 5, 0, 35, 17: an empty segment, starts off the 16-row grid, ragged last tiles
SIGMA = [0.05, 0.1, 0.2, 0.4]
CLIP = [0.0, 0.3, 0.25, 0.0]
DEC = [1e-4, 2e-4, 3e-4, 5e-4]  # per env of a launch, as Agent.action_noise_decrease
EINVAL = -22


class _Bound:
    """The agents' own exploration state (learner._explore_rng /
    exploration_noise_t / action_noise_decrease) set for a test and put back
    afterwards: the agents are shared between tests."""

    def __init__(self, agents, sigma, dec):
        self.agents = agents
        self.saved = [(a.learner.exploration_noise_t.clone(), a.learner._explore_rng.state.clone(),
                       a.learner.action_noise_decrease) for a in agents]
        for a, s, d in zip(agents, sigma, dec):
            a.learner.exploration_noise_t.fill_(s)
            a.learner.action_noise_decrease = d

    def states(self):
        return [(a.learner._explore_rng, a.learner.exploration_noise_t) for a in self.agents]

    def snap(self, p):
        L = self.agents[p].learner
        return L.exploration_noise_t.clone(), L._explore_rng.state.clone()

    def put(self, p, st):
        L = self.agents[p].learner
        L.exploration_noise_t.copy_(st[0])
        L._explore_rng.state.copy_(st[1])

    def restore(self):
        for a, (sig, rng, dec) in zip(self.agents, self.saved):
            a.learner.exploration_noise_t.copy_(sig)
            a.learner._explore_rng.state.copy_(rng)
            a.learner.action_noise_decrease = dec


def _own_select(ag, obs, clip, scale):
    """The agent's own td7f_select at 16-row tiles from its own noise state:
    FusedNets.select where that can say it (clip 0), else the very call
    FusedNets.select makes with the clip in its td7f_noise."""
    from exo_amd import _native as nat
    from exo_amd.fused import _lin_array
    L, fz = ag.learner, ag.learner.fused
    n = obs.shape[0]
    if clip == 0.0:
        return fz.select(obs, scale=scale, rt=1).clone()
    fz.refresh("fixed_encoder", "actor")
    obs = obs.contiguous()
    out = torch.empty((n, 7), dtype=torch.float32, device=obs.device)
    nz = fz._noise(L._explore_rng, L.exploration_noise_t, L.action_noise_decrease * n, clip, scale)
    fe = fz.nets["fixed_encoder"].layers
    nat.check(nat.lib().td7f_select(fz.prec, fz.act, _lin_array(fe[:3]), fz.nets["actor"].array, nat.ptr(obs), n,
                                    ctypes.byref(nz), nat.ptr(out), 0, 1, nat.stream_ptr(obs.device)), "td7f_select")
    return out


def _same_state(x, y):
    return torch.equal(_bits(x[0]), _bits(y[0])) and torch.equal(x[1], y[1])


@pytest.mark.parametrize("shape", ["default", "w256"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_each_policy_equals_its_own_select(precision, shape):
    from exo_amd.fused import MultiNoise
    agents = [_agent(precision, shape, k) for k in range(4)]
    n, scale, G = SEG[-1], 0.75, 16
    lens = [b - a for a, b in zip(SEG[:-1], SEG[1:])]
    obs = _obs(n)
    ps = _policy_set(agents)
    bound = _Bound(agents, SIGMA, DEC)
    try:
        # FusedNets.select decreases sigma by action_noise_decrease * rows: the same product here
        mn = MultiNoise(ps, None, sigma_dec=[d * ln for d, ln in zip(DEC, lens)], clip=CLIP, states=bound.states())
        for call in range(2):  # the second draws with the advanced counter and sigma
            before = [bound.snap(p) for p in range(4)]
            guard = torch.full((n + 2 * G, 7), float("nan"), device="cuda")
            out = guard[G:G + n]
            ps.act(obs, SEG, out=out, scale=scale, noise=mn)
            torch.cuda.synchronize()
            after = [bound.snap(p) for p in range(4)]
            assert bool(torch.isfinite(out).all())
            assert bool(torch.isnan(guard[:G]).all()) and bool(torch.isnan(guard[G + n:]).all())
            assert int(mn.ticket[0]) == 0
            for p, ag in enumerate(agents):
                a, b = SEG[p], SEG[p + 1]
                if b == a:  # no rows: its state is neither read nor written
                    assert _same_state(after[p], before[p]), f"call {call}: empty segment {p}"
                    continue
                bound.put(p, before[p])
                want = _own_select(ag, obs[a:b], CLIP[p], scale)
                torch.cuda.synchronize()
                assert torch.equal(_bits(out[a:b]), _bits(want)), f"call {call}: segment {p}"
                # sigma, call counter (and the rng's own ticket word, zero) as its own launch left them
                assert _same_state(after[p], bound.snap(p)), f"call {call}: noise state of policy {p}"
                assert not _same_state(after[p], before[p])
            # the noise was there
            assert not torch.equal(_bits(out), _bits(ps.act(obs, SEG, scale=scale)))
    finally:
        bound.restore()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_segment_offset_independence(precision):
    from exo_amd.fused import MultiNoise
    A, B, X = (_agent(precision, "default", k) for k in range(3))
    O = _obs(41)
    obs_far = torch.cat([O[20:41], O[:17]]).contiguous()  # X's 17 rows at 21..38
    bound = _Bound([A, B, X], [0.3, 0.2, 0.15], [0.0, 0.0, 1e-3])
    try:
        ps1, ps3 = _policy_set([X]), _policy_set([A, B, X])
        st = bound.states()
        x0 = bound.snap(2)
        near = ps1.act(O[:17].contiguous(), [0, 17], noise=MultiNoise(ps1, None, 1e-3, 0.2, states=st[2:])).clone()
        torch.cuda.synchronize()
        x1 = bound.snap(2)
        bound.put(2, x0)
        far = ps3.act(obs_far, [0, 16, 21, 38], noise=MultiNoise(ps3, None, [0.0, 0.0, 1e-3], [0.0, 0.0, 0.2],
                                                                 states=st))
        torch.cuda.synchronize()
        assert torch.equal(_bits(far[21:38]), _bits(near))
        assert _same_state(bound.snap(2), x1)
    finally:
        bound.restore()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_given_normals_closed_form(precision):
    from exo_amd.fused import MultiNoise
    agents = [_agent(precision, "default", k) for k in range(4)]
    n, scale = SEG[-1], 0.75
    obs = _obs(n)
    ps = _policy_set(agents)
    dec = [1e-3, 2e-3, 3e-3, 4e-3]
    mn = MultiNoise(ps, SIGMA, dec, CLIP)
    z = torch.randn((n, 7), generator=torch.Generator().manual_seed(11)).to("cuda")
    # t is in [-1, 1] already: the kernel's clamp of it is the identity
    t = ps.act(obs, SEG, scale=1.0).double().cpu().numpy()
    got = ps.act(obs, SEG, scale=scale, noise=mn, z=z).double().cpu().numpy()
    torch.cuda.synchronize()
    z64 = z.double().cpu().numpy()
    for p in range(4):
        a, b = SEG[p], SEG[p + 1]
        sg, cl = float(np.float32(SIGMA[p])), float(np.float32(CLIP[p]))
        e = z64[a:b] * sg
        if cl > 0:
            e = np.clip(e, -cl, cl)
        want = np.clip(t[a:b] + e, -1.0, 1.0) * scale
        # the product (or fused multiply-add), the sum and the scale: three
        # fp32 roundings of magnitudes bounded by 1 + |z| sigma
        tol = 3 * 2.0 ** -24 * (1 + np.abs(z64[a:b]) * sg) * scale
        err = np.abs(got[a:b] - want)
        print(f"policy {p}: max err / tol {float((err / tol).max()) if b > a else 0.0:.3g}")
        assert bool((err <= tol).all()), f"policy {p}"
    assert mn.counters() == [0, 0, 0, 0]  # given normals: no counter moves
    want_sigma = [np.float32(np.float32(s) - np.float32(d)) if SEG[p + 1] > SEG[p] else np.float32(s)
                  for p, (s, d) in enumerate(zip(SIGMA, dec))]
    np.testing.assert_array_equal(mn.sigma.cpu().numpy(), np.array(want_sigma, dtype=np.float32))
    assert int(mn.ticket[0]) == 0


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_zero_sigma_is_the_deterministic_mode(precision):
    from exo_amd.fused import MultiNoise
    agents = [_agent(precision, "default", k) for k in range(4)]
    obs = _obs(SEG[-1])
    ps = _policy_set(agents)
    mn = MultiNoise(ps, 0.0, clip=[0.0, 0.1, 0.0, 0.2])
    got = ps.act(obs, SEG, scale=0.75, noise=mn)
    want = ps.act(obs, SEG, scale=0.75)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want))
    assert mn.counters() == [1, 0, 1, 1]


def test_argument_errors_launch_nothing():
    from exo_amd import _native as nat
    from exo_amd.fused import MultiNoise, select_multi_noise_raw
    agents = [_agent("bf16", "default", k) for k in range(4)]
    n = SEG[-1]
    obs = _obs(n)
    ps = _policy_set(agents)
    mn = MultiNoise(ps, SIGMA, 1e-3, CLIP)
    key, tiles, nt = ps.tiles(SEG)
    segd = ps.seg_dev(SEG)
    out = torch.full((n, 7), float("nan"), device="cuda")
    Rows = nat.TD7FNoiseRow * 4

    def rows(p=None, **kw):
        r = Rows.from_buffer_copy(mn.rows)
        for k, v in kw.items():
            setattr(r[p], k, v)
        return r

    def call(r=mn.rows, table=mn.table, seg_dev=segd, ticket=mn.ticket, seg=SEG, nt=nt):
        rc = select_multi_noise_raw(ps.prec, ps.act_codes, ps.enc, ps.actor, ps.table, seg, tiles, nt, obs, n, r, table,
                                    seg_dev, ticket, None, out, 1.0)
        torch.cuda.synchronize()
        return rc

    assert call(r=None) == EINVAL
    assert call(table=None) == EINVAL
    assert call(seg_dev=None) == EINVAL
    assert call(ticket=None) == EINVAL
    assert call(r=rows(0, sigma_dec=-1e-3)) == EINVAL
    assert call(r=rows(3, clip=-0.5)) == EINVAL
    assert call(r=rows(2, sigma=None)) == EINVAL      # a row with a segment needs its state
    assert call(r=rows(0, counter=None)) == EINVAL
    assert call(seg=[0, 5, 5, 41, 57]) == EINVAL      # td7f_select_multi's own checks hold too
    assert call(nt=nt + 1) == EINVAL
    assert bool(torch.isnan(out).all())
    nat.lib().td7f_probe(1)
    try:
        assert call() == 0                            # plan-only: valid, nothing launched
    finally:
        nat.lib().td7f_probe(0)
    assert bool(torch.isnan(out).all())
    assert mn.counters() == [0, 0, 0, 0]
    # the empty segment's row may point nowhere; the host table refuses what a row cannot hold
    assert call(r=rows(1, sigma=None, counter=None)) == 0
    assert bool(torch.isfinite(out).all())
    per = (nat.TD7FNoise * 1)(nat.TD7FNoise(1, 2, 0, None, None, None, 0.0, 0.0, 1.0, 0, mn.table.data_ptr(), None))
    assert nat.lib().td7f_multi_noise_table(1, per, Rows()) == EINVAL
    with pytest.raises(ValueError, match="sigma"):
        MultiNoise(ps, [0.1, 0.2])
    with pytest.raises(ValueError, match="clip"):
        MultiNoise(ps, 0.1, clip=-1.0)
    with pytest.raises(ValueError, match="distinct"):
        MultiNoise(ps, 0.1, tags=[7, 8, 7, 9])
    with pytest.raises(ValueError, match="policies"):
        _policy_set(agents[:2]).act(obs[:40], [0, 24, 40], noise=mn)


def test_capture_replays_equal_eager_launches():
    from exo_amd import graphs
    from exo_amd.fused import MultiNoise
    agents = [_agent("bf16", "default", k) for k in range(4)]
    n = SEG[-1]
    obs = _obs(n)
    ps = _policy_set(agents)
    mn = MultiNoise(ps, SIGMA, [1e-3, 2e-3, 3e-3, 4e-3], CLIP)
    out = torch.empty((n, 7), device="cuda")
    eager = []
    for _ in range(3):
        ps.act(obs, SEG, out=out, scale=0.75, noise=mn)
        eager.append(out.clone())
    torch.cuda.synchronize()
    sigma_e, count_e = mn.sigma.clone(), mn.counters()
    assert count_e == [3, 0, 3, 3]
    mn.sigma.copy_(torch.tensor(SIGMA, device="cuda"))
    for r in mn.rngs:
        r.state.zero_()
    cur = torch.cuda.current_stream()
    s = torch.cuda.Stream()
    s.wait_stream(cur)
    g = graphs.new_graph()
    try:
        with torch.cuda.stream(s):
            with graphs.capture(g, stream=s):
                ps.act(obs, SEG, out=out, scale=0.75, noise=mn)
        cur.wait_stream(s)
        assert mn.counters() == [0, 0, 0, 0]  # recorded, not run
        for k in range(3):
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(out), _bits(eager[k])), f"replay {k}"
        assert torch.equal(_bits(mn.sigma), _bits(sigma_e)) and mn.counters() == count_e
        assert int(mn.ticket[0]) == 0
    finally:
        graphs.release_graphs(g)
