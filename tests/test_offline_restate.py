"""The offline (TD3+BC, Agent/TD7_multi_agent.py:272-274) actor update of the
torch-autograd branch as an fp64 reference, and what that reference says about
the cases tests/test_offline_fused_gpu.py runs on the GPU -- on the CPU alone.

* TD7Learner.phase_actor_grads with offline=True runs on td7_restate._f64_learner
  and returns fp64 gradients (it raised "Found dtype Double but expected Float":
  actor.float() against an fp64 action inside F.mse_loss).
* With fp32 inputs and offline=False the gradients are those of
  torch.autograd.grad(-Q.float().mean(), params), written out here.
* For every GPU case, from the perturbed initial state (td7_restate
  .perturbed_cpu_learner with the case's Q bounds) and the batch of the step
  that updates the actor:
    (i)  on each actor tensor the offline and the online restated gradients
         differ by rel L2 >= 0.3 at lmbda = 1.0 and >= 0.03 at lmbda = 0.1
         (||offline - online|| over the larger of the two norms), and
    (ii) 2 * flip <= td7_restate.FLIP_CAP,
  so a kernel that drops or mis-scales the BC term cannot pass inside the GPU
  test's bounds (at most max(1e-2, 2 flip) <= 3e-2 there).
"""
import numpy as np
import pytest
import torch

from td7_restate import (FLIP_CAP, Restatement, _cpu_learner, _f64_learner, case_qbounds, perturbed_cpu_learner,
                         td7_batch, width_hp)

# (precision, width, B, lmbda): each B is the smallest that reaches its edge (td7_restate.CASES)
OFFLINE_CASES = [("fp32", None, 17), ("fp32", 256, 250), ("bf16", None, 1), ("bf16", None, 250), ("bf16", 256, 17),
                 ("fp16", 256, 40), ("fp16", None, 264)]
ALL_CASES = [c + (1.0,) for c in OFFLINE_CASES] + [("bf16", None, 264, 0.1)]
MIN_DIFF = {1.0: 0.3, 0.1: 0.03}


def offline_hp(width, lmbda):
    hp = width_hp(width)
    hp.lmbda = lmbda
    return hp


def offline_restatement(hp, precision, offline=True):
    """td7_restate.Restatement with every arm an offline learner."""
    R = Restatement(hp, precision)
    for L, _, _ in R.arms.values():
        L.offline = offline
    return R


def test_the_offline_branch_restates_in_fp64():
    hp = offline_hp(None, 1.0)
    L = _f64_learner(hp)
    L.offline = True
    s, a = (torch.tensor(x, dtype=torch.float64) for x in td7_batch(17, 1)[:2])
    L._fixed_zs = L.fixed_encoder.zs(s).detach()
    L.phase_actor_grads(s, a)
    for n, p in L.actor.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float64, n
        assert torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
    # the loss written out in fp64
    actor = L.actor(s, L._fixed_zs)
    Q = L.critic(s, actor, L.fixed_encoder.zsa(L._fixed_zs, actor), L._fixed_zs)
    assert Q.dtype == torch.float64
    loss = -Q.mean() + hp.lmbda * Q.abs().mean().detach() * ((actor - a) ** 2).mean()
    ref = torch.autograd.grad(loss, list(L.actor.parameters()))
    for (n, p), g in zip(L.actor.named_parameters(), ref):
        torch.testing.assert_close(p.grad, g, rtol=1e-12, atol=1e-15, msg=lambda m: f"{n}: {m}")


def test_the_online_fp32_gradients_are_unchanged():
    hp = width_hp(None)
    L = _cpu_learner(hp)
    assert not L.offline
    s, a = (torch.tensor(x) for x in td7_batch(17, 1)[:2])
    L._fixed_zs = L.fixed_encoder.zs(s).detach()
    L.phase_actor_grads(s, a)
    actor = L.actor(s, L._fixed_zs)
    Q = L.critic(s, actor, L.fixed_encoder.zsa(L._fixed_zs, actor), L._fixed_zs)
    ref = torch.autograd.grad(-Q.float().mean(), list(L.actor.parameters()))
    for (n, p), g in zip(L.actor.named_parameters(), ref):
        assert p.grad.dtype == torch.float32
        assert torch.equal(p.grad, g), n


@pytest.mark.parametrize("precision,width,B,lmbda", ALL_CASES)
def test_the_reference_separates_the_bc_term(precision, width, B, lmbda):
    hp = offline_hp(width, lmbda)
    state = perturbed_cpu_learner(hp, case_qbounds(precision, width, B))
    batch = td7_batch(B, 1)
    Roff = offline_restatement(hp, precision)
    noise, flip = Roff.actor(state, batch)
    off = Roff.grads(Roff.ref, ("actor",))
    Ron = offline_restatement(hp, precision, offline=False)
    Ron.arms = {"ref": Ron.arms["r64" if "r64" in Ron.arms else "f64"]}
    Ron.actor(state, batch)
    on = Ron.grads(Ron.ref, ("actor",))
    assert set(off) == set(on) == set(flip)
    for name in off:
        d = np.linalg.norm(off[name] - on[name]) / max(np.linalg.norm(off[name]), np.linalg.norm(on[name]))
        print(f"  {name}: offline vs online {d:.3g} noise {noise[name]:.2e} flip {flip[name]:.2e}")
        assert d >= MIN_DIFF[lmbda], f"{name}: the BC term moves the gradient by {d:.3g} only"
        assert 2 * flip[name] <= FLIP_CAP, f"{name}: flip {flip[name]:.3g}"
