"""td7f::wgrad_kernel's layout choices (csrc/td7_fused_train.hip) change which
workgroup or thread touches which bytes, never a value:

  EXO_WGRAD_XCD  tiles in XCD-contiguous order (csrc/td7_xcd_map.h) or in
                 blockIdx.x order;
  EXO_WGRAD_VEC  dW and the Adam state as 16-byte row accesses through an
                 fp32 LDS tile, or one dword per lane in the accumulator layout.

Every arm must leave td7f_wgrad's and td7f_wgrad_adam's outputs bit for bit
those of the (identity order, scalar) arm: every dW and db, p / m / v and the
step counts, every packed wf / wb, the LAP priorities.  The scalar arm is
itself pinned to td7f_wgrad + td7f_adam_pack by tests/test_adam_pack_gpu.py.

Shapes: the bench's nets at bf16 (135 / 230 / 90 tiles, no multiple of 8;
K = 87 and K = 307 stay scalar in the vector arms, K = 300 leaves a 44-wide
last k-tile) and the 256-wide nets at fp16; B = 40 (rows padded to 256); a
one-job launch of 5 tiles (fewer than the 8 XCDs)."""
import pytest
import torch

from exo_amd import _native as nat
from exo_amd.td7 import Hyperparameters, TD7Learner

pytestmark = pytest.mark.gpu

B = 40
REF = ("0", "0")  # (EXO_WGRAD_XCD, EXO_WGRAD_VEC): the layout before either choice
ARMS = [("1", "0"), ("0", "1"), ("1", "1")]


def _learner(precision, width):
    torch.manual_seed(7)
    hp = Hyperparameters() if width is None else Hyperparameters(zs_dim=width, enc_hdim=width, critic_hdim=width,
                                                                 actor_hdim=width)
    L = TD7Learner(80, 7, hp, device="cuda", precision=precision)
    assert L.fused is not None
    return L


def _tensors(opt, net):
    out = [opt.flat, opt.m, opt.v, opt._step]
    for pl in net.layers:
        out.append(pl.wf)
        if pl.wb is not None:
            out.append(pl.wb)
    return out


def _batch(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    s = torch.randn(B, 80, device="cuda", generator=g)
    a = torch.rand(B, 7, device="cuda", generator=g) * 2 - 1
    ns = torch.randn(B, 80, device="cuda", generator=g)
    r = torch.randn(B, 1, device="cuda", generator=g)
    nd = torch.ones(B, 1, device="cuda")
    return s, a, ns, r, nd


def _run(monkeypatch, arm, launch, state, before, outs):
    """State restored to `before`, outputs poisoned, one launch under `arm`;
    returns clones of state + outs."""
    monkeypatch.setenv("EXO_WGRAD_XCD", arm[0])
    monkeypatch.setenv("EXO_WGRAD_VEC", arm[1])
    for t, b in zip(state, before):
        t.copy_(b)
    for t in outs:
        t.fill_(float("nan"))
    launch()
    return [t.clone() for t in state + outs]


def _check_arms(monkeypatch, what, launch, state, outs):
    before = [t.clone() for t in state]
    ref = _run(monkeypatch, REF, launch, state, before, outs)
    assert not any(torch.isnan(t).any() for t in ref[len(state):]), f"{what}: an output was not written"
    for arm in ARMS:
        got = _run(monkeypatch, arm, launch, state, before, outs)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), f"{what} XCD={arm[0]} VEC={arm[1]}: tensor {k} differs"


@pytest.mark.parametrize("precision,width", [("bf16", None), ("fp16", 256)])
def test_wgrad_layout_arms_are_bit_identical(monkeypatch, precision, width):
    L = _learner(precision, width)
    F = L.fused
    tr = F.train(B)
    assert tr.fuses_adam() and tr.ld == 256
    cases = [("encoder", L.encoder_optimizer, tr.wgrad_encoder, tr.enc_grad, []),
             ("critic", L.critic_optimizer, tr.wgrad_critic, tr.critic_grad, [tr.prio]),
             ("actor", L.actor_optimizer, tr.wgrad_actor, tr.actor_grad, [])]
    if width is None:
        tiles = {n: sum(-(-j.n // 64) * -(-j.k // 64) for j in jobs)
                 for n, jobs in (("encoder", tr.jobs_e), ("critic", tr.jobs_c), ("actor", tr.jobs_a))}
        assert tiles == {"encoder": 135, "critic": 230, "actor": 90}
    with torch.no_grad():
        for step in range(3):  # moments and bias corrections away from their first-step values
            batch = _batch(step)
            L.phase_grads(*batch)  # fills the transposed operands of every layer
            L.phase_actor_grads(batch[0], batch[1])
            for name, opt, wgrad, grad, extra in cases:
                state = _tensors(opt, F.nets[name])
                _check_arms(monkeypatch, f"step {step} {name} wgrad", lambda: wgrad(adam=False), state, [grad] + extra)
                # last: leaves the stepped state for the next step
                _check_arms(monkeypatch, f"step {step} {name} wgrad_adam", lambda: wgrad(adam=True), state,
                            [grad] + extra)
    assert all(float(opt._step) == 3.0 for _, opt, _, _, _ in cases)


def test_single_job_with_fewer_tiles_than_xcds(monkeypatch):
    """The actor's l3 alone: N = 7, K = 320 -- 5 tiles on 8 XCDs."""
    L = _learner("bf16", None)
    F = L.fused
    tr = F.train(B)
    i = next(i for i, j in enumerate(tr.jobs_a) if j.n == 7)
    assert tr.jobs_a[i].k == 320
    jobs = (nat.TD7FWgJob * 1)(tr.jobs_a[i])
    descs = (nat.TD7FWgAdam * 1)(tr.adam_a[i])
    opt = L.actor_optimizer
    state = _tensors(opt, F.nets["actor"])
    with torch.no_grad():
        for step in range(3):
            batch = _batch(10 + step)
            L.phase_grads(*batch)
            L.phase_actor_grads(batch[0], batch[1])
            act_p = list(L.actor.parameters())
            outs = [act_p[2 * i].grad, act_p[2 * i + 1].grad]
            _check_arms(monkeypatch, f"step {step} l3 wgrad", lambda: tr._wgrad(jobs, descs, opt, False), state, outs)
            _check_arms(monkeypatch, f"step {step} l3 wgrad_adam", lambda: tr._wgrad(jobs, descs, opt, True), state,
                        outs)
    assert float(opt._step) == 3.0
