"""td7f_select_multi_seq / PolicySet.act(noise=PinkNoise) on the MI355X: the
multi-policy select launch with each env's own column of its coloured noise
sequence (TD7_multi_agent_Pink_noise.py:203-228 per env).

The kernel runs select_multi_kernel's rows and adds a term it only loads, so
its output equals the deterministic launch followed by the same three fp32
operations in torch, bit for bit.  Policies, observations: test_select_multi_gpu.py's.
"""
import numpy as np
import pytest
import torch

from test_select_multi_gpu import _agent, _bits, _obs, _policy_set

pytestmark = pytest.mark.gpu

SEG = [0, 5, 5, 38]  # an empty segment, a start off the 16-row grid, ragged last tiles
SIGMA = [0.2, 0.1, 0.4]
DEC = [1e-3, 2e-3, 3e-3]
CLIP = [0.0, 0.0, 0.15]
SCALE = 0.75


def _lengths(n):
    ln = np.random.default_rng(4).choice([232, 347, 288, 17], size=n)
    ln[:3] = (347, 17, 232)
    return ln


def _setup(precision):
    from exo_amd.fused import PinkNoise
    agents = [_agent(precision, "default", k) for k in range(3)]
    ps = _policy_set(agents)
    n = SEG[-1]
    ln = _lengths(n)
    pn = PinkNoise(ps, SEG, ln, SIGMA, DEC, CLIP)
    # mixed step indices: the first step, the last column of a row (t = n_r - 1), and in between
    t = np.random.default_rng(6).integers(0, ln)
    t[0], t[1], t[5], t[37] = 0, ln[1] - 1, ln[5] - 1, ln[37] - 1
    pn.t.copy_(torch.as_tensor(t.astype(np.int32)))
    return ps, pn, _obs(n), t


def _want(ps, pn, obs, t):
    a = ps.act(obs, SEG)  # deterministic, scale 1: tanh(.) in [-1, 1]
    e = pn.seq[torch.arange(pn.n, device="cuda"), torch.as_tensor(t, device="cuda")]
    for p in range(3):
        if CLIP[p] > 0:
            e[SEG[p]:SEG[p + 1]] = e[SEG[p]:SEG[p + 1]].clamp(-CLIP[p], CLIP[p])
    return torch.clamp(a + e, -1.0, 1.0) * SCALE, e


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_equals_the_deterministic_launch_plus_the_sequence_column(precision):
    ps, pn, obs, t = _setup(precision)
    n, G = SEG[-1], 16
    want, e = _want(ps, pn, obs, t)
    assert bool((e.abs() > 0).any(1).all())  # every row has a noise term
    assert bool((pn.seq[33:38].abs().max() > CLIP[2]))  # and the clip has something to cut
    sigma0, counters0 = pn.sigma.clone(), [r.state.clone() for r in pn.rngs]
    seq0, t0 = pn.seq.clone(), pn.t.clone()
    guard = torch.full((n + 2 * G, 7), float("nan"), device="cuda")
    out = guard[G:G + n]
    ps.act(obs, SEG, out=out, scale=SCALE, noise=pn)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    assert bool(torch.isnan(guard[:G]).all()) and bool(torch.isnan(guard[G + n:]).all())
    assert not torch.equal(_bits(out), _bits(ps.act(obs, SEG, scale=SCALE)))
    # sigma of the policies with rows drops by sigma_dec; nothing else moves
    s0 = sigma0.cpu().numpy()
    want_sigma = [np.float32(s0[p] - np.float32(DEC[p])) if SEG[p + 1] > SEG[p] else s0[p] for p in range(3)]
    np.testing.assert_array_equal(pn.sigma.cpu().numpy(), np.array(want_sigma, dtype=np.float32))
    for r, c in zip(pn.rngs, counters0):
        assert torch.equal(r.state, c)
    assert int(pn.ticket[0]) == 0
    assert torch.equal(_bits(pn.seq), _bits(seq0)) and torch.equal(pn.t, t0)
    # a second launch without advance: the same noise terms (sigma is frozen in the sequence)
    again = ps.act(obs, SEG, scale=SCALE, noise=pn)
    torch.cuda.synchronize()
    assert torch.equal(_bits(again), _bits(out))
    assert pn.sigma.cpu().numpy()[0] == np.float32(want_sigma[0] - np.float32(DEC[0]))


def test_step_index_is_clamped_to_the_table():
    ps, pn, obs, t = _setup("bf16")
    pn.t[3] = pn.Lmax + 5
    pn.t[4] = -2
    t = t.copy()
    t[3], t[4] = pn.Lmax - 1, 0
    want, _ = _want(ps, pn, obs, t)
    out = ps.act(obs, SEG, scale=SCALE, noise=pn)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
