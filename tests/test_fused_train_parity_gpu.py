"""The fused gradient passes (csrc/td7_fused_train.hip: td7f_encoder,
td7f_critic_phase, td7f_actor, td7f_wgrad) against an independent reference at
ragged and tiny batches, the 256-wide tile class (4 tiles per wave) and fp16 --
shapes at which they were only ever compared with each other.

Cases (tests/td7_restate.py CASES): fp32 / bf16 / fp16 x the default widths
(300 / 320) and 256 x B in {1, 17, 40, 250, 264}: one row; a 16-row tile plus
one row; tests/test_wgrad_layout_gpu.py's shape; ld = 256 with a last tile of
10 rows (exactly 8 k-steps at 16 bits, the weight-gradient kernel's prefetch
distance); ld = 512 with a last tile of 8 rows.  Two teacher-forced steps each,
as tests/test_td7_full.py runs them; the second updates the actor and starts
from the running Q bounds the first one left.  The Q-target clamp is set to the
quartiles of the first batch's target values (td7_restate.case_qbounds), so it
binds on about half of the rows (tests/test_td7_restate.py asserts 10..90 %).

(a) td7f_wgrad against its own stored operands.  Every layer's X^T / dP^T
    (exo_amd/fused.py XTBuffers) is decoded (td7_restate.unblock_xt) and
      dW_ref = dP^T[:, :B] X^T[:, :B]^T / gs      (fp64; gs = 1024 at fp16)
    must match the parameter's gradient to rtol 1e-4, atol 1e-4 max|dW_ref| --
    the per-layer kernels' bound for "the fp64 GEMM of the stored operands"
    (tests/test_td7_dense_gpu.py), without its floor of 1: these gradients
    carry a 1/B factor.  The padding must be what include/exo_amd.h promises:
    dP^T zero in every batch row >= B (the phantom rows of the last tile
    included, whose X^T holds act(bias), not zero), both operands zero in the
    operand rows beyond N / K, and dP^T[:, B:] X^T[:, B:]^T exactly zero.  The
    bias gradient is the sum of the per-tile column partials (rtol 1e-5, atol
    1e-5 max|ref|), the LAP priorities max(td0, td1, min_priority)^alpha of
    the stored |td| (1e-5).
    Observed on the MI355X: rel(dW, dW_ref) <= 3.1e-7 (fp32), 8.5e-8 (bf16),
    1.2e-7 (fp16), exactly 0 at B = 1; rel(db) <= 1.3e-7; priorities within
    1.1e-7.

(b) End to end against this step's fp64 restatement from the GPU learner's
    own state (td7_restate.Restatement; at bf16 / fp16 under _rounded_matmuls),
    every gradient tensor whole, rel = ||g - ref|| / ||ref||:
      fp32:         max(1e-4, 4 noise)
      bf16 / fp16:  max(1e-2, 4 noise sqrt(u / 1e-7), 2 flip)
    -- tests/test_td7_full.py's bound against "this step's rounded
    restatement", plus the flip term: flip = rel(fp32-accumulating rounded
    restatement, fp64-accumulating one) is what the accumulation order alone
    does to a gradient once activations are re-rounded to 16 bits, measured on
    the CPU reference, never on the kernels; the GPU's order is a second,
    independent draw of the same process, hence the factor 2
    (tests/test_td7_restate.py caps 2 flip at 3e-2).  |td| (upstream of every
    critic gradient): 1e-5 elementwise at fp32, rel L2 <= 1e-2 at 16 bits; the
    running Q bounds within 1e-5 / 1e-2 x max(1, |ref|); target_policy_noise
    within 1e-7.
    Observed on the MI355X: rel <= 1.3e-6 (fp32), 6.2e-3 (bf16: the actor's
    tensors at B = 1, flip ~ 0 there; <= 2.8e-3 at the larger batches), 4.9e-3
    (fp16: actor.l0.weight at B = 264, its flip 4.6e-3); |td| rel <= 1.2e-7 /
    3.2e-4 / 3.1e-5.  On the reference: flip <= 5.5e-3 (fp16, 256 wide,
    B = 250); noise <= 2e-6 on every tensor but four, all at step 2: 4.2e-4 /
    2.8e-4 on critic.q01.weight / .bias (fp16, 256 wide, B = 40) and 2.4e-4 /
    3.7e-5 on actor.l0.weight / .bias (bf16, default widths, B = 250), where
    the kernels were 2.2e-4 / 1.4e-4 and 2.8e-3 / 3.9e-4 from the restatement.
"""
import numpy as np
import pytest
import torch

from helpers import TD7_FULL_LEARNING_STEPS
from td7_restate import (AMP, CASES, COND, NETS, STEPS, TOL, Restatement, _rel, case_qbounds, perturbed_cpu_learner,
                         td7_batch, unblock_xt, width_hp)
from exo_amd.td7 import TD7Learner

pytestmark = pytest.mark.gpu

ENC = ("zs1", "zs2", "zs3", "zsa1", "zsa2", "zsa3")
ACTOR = ("l0", "l1", "l2", "l3")


def _learner(precision, width, B):
    """The case's learner on the GPU, as tests/test_fused_gpu.py builds its
    own (fused fp32 operands on, target / fixed nets and the actor perturbed,
    packed), from the CPU initial state the reference-only tests use."""
    from exo_amd import fused
    hp = width_hp(width)
    qb = case_qbounds(precision, width, B)
    C = perturbed_cpu_learner(hp, qb)
    f0 = fused.FUSED_F32
    fused.FUSED_F32 = precision == "fp32"  # read when the learner builds its fused nets
    try:
        L = TD7Learner(80, 7, hp, learning_steps=TD7_FULL_LEARNING_STEPS, device="cuda", precision=precision)
    finally:
        fused.FUSED_F32 = f0
    for name in NETS:
        getattr(L, name).load_state_dict(getattr(C, name).state_dict())
    L.min_target.fill_(qb[0])
    L.max_target.fill_(qb[1])
    L.max.fill_(-1e8)
    L.min.fill_(1e8)
    assert L.fused is not None and L.fused_train, getattr(L.fused, "train_error", "the per-layer kernels run it")
    L.fused.pack_all()
    return L


def _layers(L, tr, which):
    """(name, XTBuffers, dW, db) of every layer a pass trains."""
    out = []
    if which == "encoder":
        for n, xb in zip(ENC, tr.xt_enc):
            lin = getattr(L.encoder, n)
            out.append((f"encoder.{n}", xb, lin.weight.grad, lin.bias.grad))
    elif which == "critic":
        for k in range(4):
            gw, gb = getattr(L.critic, f"w{k}").grad, getattr(L.critic, f"b{k}").grad
            for h in range(2):
                out.append((f"critic.w{k}[{h}]", tr.xt_critic[2 * k + h], gw[h], gb[h]))
    else:
        for n, xb in zip(ACTOR, tr.xt_actor):
            lin = getattr(L.actor, n)
            out.append((f"actor.{n}", xb, lin.weight.grad, lin.bias.grad))
    return out


def _check_operands(L, tr, which, B, precision, step, obs):
    """(a): the weight / bias gradients of one pass from its stored operands."""
    gs = 1024.0 if precision == "fp16" else 1.0
    ld = tr.ld
    assert ld == -(-B // 256) * 256
    for name, xb, gw, gb in _layers(L, tr, which):
        at = f"step {step} {name}"
        N, K = xb.N, xb.K
        assert tuple(gw.shape) == (N, K) and tuple(gb.shape) == (N,), at
        Xf = unblock_xt(xb.x, xb.x.shape[0], ld, precision)
        DPf = unblock_xt(xb.dp, xb.dp.shape[0], ld, precision)
        X, DP = Xf[:K], DPf[:N]
        assert torch.isfinite(Xf).all() and torch.isfinite(DPf).all(), at
        assert not Xf[K:].any(), f"{at}: X^T is not zero in the operand rows beyond K"
        assert not DPf[N:].any(), f"{at}: dP^T is not zero in the operand rows beyond N"
        nz = DP[:, B:].nonzero()
        assert nz.numel() == 0, f"{at}: dP^T is not zero at (column, batch row - B) {nz[:4].tolist()}"
        assert not (DP[:, B:] @ X[:, B:].T).any(), f"{at}: the padding contributes to dW"
        ref = DP[:, :B] @ X[:, :B].T / gs
        g = gw.detach().double().cpu()
        top = float(ref.abs().max())
        if top == 0.0:
            assert not g.any(), f"{at}: dW must be zero"
        else:
            rel = float((g - ref).norm() / ref.norm())
            obs["a.dW"] = max(obs.get("a.dW", 0.0), rel)
            torch.testing.assert_close(g, ref, rtol=1e-4, atol=1e-4 * top,
                                       msg=lambda m: f"{at}: dW (rel {rel:.3g}) {m}")
        assert tuple(xb.part.shape) == (-(-B // 16), N)
        bref = xb.part.detach().double().sum(0).cpu()
        b = gb.detach().double().cpu()
        btop = float(bref.abs().max())
        if btop > 0:
            obs["a.db"] = max(obs.get("a.db", 0.0), float((b - bref).norm() / bref.norm()))
        torch.testing.assert_close(b, bref, rtol=1e-5, atol=1e-5 * btop, msg=lambda m: f"{at}: db {m}")


def _check_grads(L, R, mnames, noise, flip, precision, step, obs):
    """(b): every gradient tensor of the nets `mnames` against the restatement."""
    got, ref = R.grads(L, mnames), R.grads(R.ref, mnames)
    assert set(got) == set(ref) == set(noise) == set(flip)
    bad = []
    for name, r in ref.items():
        rel = _rel(got[name], r)
        bound = max(TOL[precision]["grad"], COND * noise[name] * AMP[precision])
        if precision != "fp32":
            bound = max(bound, 2 * flip[name])
        obs["b.grad"] = max(obs.get("b.grad", 0.0), rel)
        obs["noise"] = max(obs.get("noise", 0.0), noise[name])
        obs["flip"] = max(obs.get("flip", 0.0), flip[name])
        print(f"  step {step} {name}: rel {rel:.2e} bound {bound:.2e} noise {noise[name]:.2e} flip {flip[name]:.2e}")
        if not rel <= bound:
            bad.append(f"{name}: rel {rel:.3g} > {bound:.3g} (noise {noise[name]:.3g}, flip {flip[name]:.3g})")
    assert not bad, f"step {step} gradients vs the fp64 restatement ({precision}): " + "; ".join(bad)


def _in(t, flat):
    """t is a view into the flat buffer."""
    return flat.data_ptr() <= t.data_ptr() < flat.data_ptr() + flat.numel() * flat.element_size()


@pytest.mark.parametrize("precision,width,B", CASES)
def test_fused_gradient_passes_match_the_restatement(precision, width, B):
    L = _learner(precision, width, B)
    hp = L.hp
    R = Restatement(hp, precision)
    tol = TOL[precision]
    obs = {}
    for step in range(STEPS):
        batch = td7_batch(B, step)
        b = [torch.tensor(x, device="cuda") for x in batch]
        noise, flip = R.critic(L, batch)  # from L's state before the step (weights, running bounds, sigma)
        L.training_steps += 1
        prio = L.phase_grads(*b[:5], noise=b[5])
        torch.cuda.synchronize()  # the passes run on side streams
        assert L.fused_train
        tr = L.fused.train(B)
        assert _in(L.encoder.zs1.weight.grad, tr.enc_grad) and _in(L.critic.w0.grad, tr.critic_grad)
        # (a)
        _check_operands(L, tr, "encoder", B, precision, step, obs)
        _check_operands(L, tr, "critic", B, precision, step, obs)
        td = tr.td.detach().double().cpu()
        assert td.shape == (B, 2) and prio.data_ptr() == tr.prio.data_ptr()
        pref = td.max(1)[0].clamp(min=hp.min_priority) ** hp.alpha
        np.testing.assert_allclose(tr.prio.double().cpu().numpy(), pref.numpy(), rtol=1e-5, atol=1e-5)
        obs["a.prio"] = max(obs.get("a.prio", 0.0), float((tr.prio.double().cpu() - pref).abs().max()))
        # (b)
        r_td = _rel(td.numpy(), R.td.numpy())
        obs["b.td"] = max(obs.get("b.td", 0.0), r_td)
        if precision == "fp32":
            np.testing.assert_allclose(td.numpy(), R.td.numpy(), rtol=1e-5, atol=1e-5)
        else:
            assert r_td <= tol["grad"], f"step {step}: |td| rel {r_td:.3g}"
        for key in ("max", "min"):
            val, ref = float(getattr(L, key)), float(getattr(R.ref, key))
            bnd = 1e-5 if precision == "fp32" else tol["grad"]
            assert abs(ref) < 1e7, (key, ref)  # the restatement saw a target
            assert abs(val - ref) <= bnd * max(1.0, abs(ref)), (step, key, val, ref)
        assert abs(float(L.target_policy_noise) - float(R.ref.target_policy_noise)) < 1e-7
        _check_grads(L, R, ("encoder", "critic"), noise, flip, precision, step, obs)
        L.phase_steps()
        if L.training_steps % hp.policy_freq == 0:
            noise, flip = R.actor(L, batch)  # the just-updated critic
            L.phase_actor_grads(b[0], b[1])
            torch.cuda.synchronize()
            assert _in(L.actor.l0.weight.grad, tr.actor_grad)
            _check_operands(L, tr, "actor", B, precision, step, obs)
            _check_grads(L, R, ("actor",), noise, flip, precision, step, obs)
            L.phase_actor_step()
    assert L.training_steps == STEPS and STEPS % hp.policy_freq == 0  # the actor pass ran
    torch.cuda.synchronize()
    print("observed", precision, width, B, {k: f"{v:.2e}" for k, v in sorted(obs.items())})
