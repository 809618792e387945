"""tests/td7_restate.py on the CPU: the weight-gradient operand decoder, and
the conditions on the reference alone that keep the bounds of
tests/test_fused_train_parity_gpu.py honest.

For every (precision, widths, B) case of that module, both steps run on the
CPU learners only (the fp32 learner carries the state from step to step; no
kernel is involved):
* every gradient tensor of the fp64 restatement is non-zero -- a relative
  error against it means something;
* with B >= 17 the Q-target clamp binds on 10 % .. 90 % of the rows
  (case_qbounds: the quartiles of the first batch's min-head target values);
* 2 * flip <= 3e-2 (the 16-bit "golden" tolerance of tests/test_td7_full.py)
  for every tensor: the flip term may lift a GPU bound only that far.
Observed over the 12 cases: flip <= 5.6e-3 (fp16, default widths, B = 264),
noise <= 1.7e-6 but for 2.4e-4 on one tensor (bf16, default widths, B = 250,
step 2), the clamp on 33 % .. 80 % of the rows with B >= 17.
"""
import numpy as np
import pytest
import torch

from td7_restate import (CASES, FLIP_CAP, STEPS, Restatement, case_qbounds, clamp_fraction, noise_and_flip,
                         perturbed_cpu_learner, td7_batch, unblock_xt, width_hp, xt_index)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("ld", [256, 512])
@pytest.mark.parametrize("rows64", [64, 128, 960])
def test_xt_index_is_a_permutation(precision, rows64, ld):
    idx = xt_index(rows64, ld, precision)
    assert idx.shape == (rows64, ld)
    assert torch.equal(idx.reshape(-1).sort()[0], torch.arange(rows64 * ld))


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
def test_unblock_xt_decodes_the_documented_layout(precision):
    """Element (c, r) written where csrc/td7_fused.h documents it comes back
    at [c, r]: blocks of 16 operand rows x 32 (fp32: 16) batch rows, the lane
    (c % 16) + 16 * (batch-row group), 8 (4) consecutive batch rows per lane."""
    rows64, ld = 128, 512
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[precision]
    kd, per = (16, 4) if precision == "fp32" else (32, 8)
    buf = torch.zeros(rows64 * ld, dtype=dt)
    want = torch.zeros(rows64, ld, dtype=torch.float64)
    for n, (c, r) in enumerate([(0, 0), (1, 0), (0, 1), (15, per - 1), (16, per), (17, kd), (127, 511), (70, 263)]):
        block = (c // 16) * (ld // kd) + r // kd
        lane = c % 16 + 16 * ((r % kd) // per)
        buf[block * 16 * kd + lane * per + r % per] = n + 1
        want[c, r] = n + 1
    raw = buf if precision == "fp32" else buf.view(torch.int16)
    assert torch.equal(unblock_xt(raw.view(rows64, ld), rows64, ld, precision), want)


def test_batches_are_keyed_and_terminal_rows_exist():
    a, b = td7_batch(264, 0), td7_batch(264, 0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], td7_batch(264, 1)[0])
    assert not np.array_equal(a[0][:250], td7_batch(250, 0)[0])
    s, act, s2, r, nd, nz = a
    assert s.shape == s2.shape == (264, 80) and act.shape == nz.shape == (264, 7) and r.shape == nd.shape == (264, 1)
    assert r.min() >= -2 and r.max() <= 3 and np.abs(act).max() <= 1
    assert 0.03 < 1 - nd.mean() < 0.2 and set(np.unique(nd)) == {0.0, 1.0}


@pytest.mark.parametrize("precision,width,B", CASES)
def test_reference_conditions_of_the_parity_cases(precision, width, B):
    hp = width_hp(width)
    qb = case_qbounds(precision, width, B)
    L = perturbed_cpu_learner(hp, qb)  # carries the state: the plain fp32 CPU update
    R = Restatement(hp, precision)
    worst = dict(noise=0.0, flip=0.0)

    def check(noise, flip, mnames, step):
        ref = R.grads(R.ref, mnames)
        assert set(ref) == set(noise) == set(flip)
        for name, g in ref.items():
            assert np.linalg.norm(g) > 0, f"step {step}: {name} is zero in the restatement"
            assert np.isfinite(noise[name]) and np.isfinite(flip[name]), name
            assert 2 * flip[name] <= FLIP_CAP, f"step {step}: {name} flip {flip[name]:.3g}"
            if precision == "fp32":
                assert flip[name] == 0.0
            worst["noise"], worst["flip"] = max(worst["noise"], noise[name]), max(worst["flip"], flip[name])

    for step in range(STEPS):
        batch = td7_batch(B, step)
        b = [torch.tensor(x) for x in batch]
        check(*R.critic(L, batch), ("encoder", "critic"), step)
        assert R.td.shape == R.heads.shape == (B, 2)
        frac = clamp_fraction(R.heads, batch[4], qb)
        if B >= 17:
            assert 0.1 <= frac <= 0.9, f"step {step}: the clamp binds on {frac:.0%} of the rows"
        L.training_steps += 1
        L.phase_grads(*b[:5], noise=b[5])
        L.phase_steps()
        if L.training_steps % hp.policy_freq == 0:
            check(*R.actor(L, batch), ("actor",), step)
            L.phase_actor_grads(b[0], b[1])
            L.phase_actor_step()
        print(f"{precision} {width} B={B} step {step}: clamp {frac:.2f} noise {worst['noise']:.2e} "
              f"flip {worst['flip']:.2e}")
    assert L.training_steps == STEPS and STEPS % hp.policy_freq == 0  # the actor's tensors were measured


def test_noise_and_flip_is_the_restatement_of_one_phase():
    """The one-call form: the same figures as a Restatement's critic phase,
    flip zero at fp32 and non-zero at bf16."""
    hp = width_hp(256)
    L = perturbed_cpu_learner(hp, case_qbounds("bf16", 256, 17))
    batch = td7_batch(17, 0)
    noise, flip = noise_and_flip(hp, batch, L, "bf16")
    n2, f2 = Restatement(hp, "bf16").critic(L, batch)
    assert noise == n2 and flip == f2
    assert max(flip.values()) > 0 and 0 < max(noise.values()) < 1e-4
    n32, f32 = noise_and_flip(hp, batch, L, "fp32")
    assert n32 == noise and set(f32.values()) == {0.0}
