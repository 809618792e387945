"""Bit fixture of the fused TD7 passes (csrc/td7_fused.hip, td7_fused_train.hip).

run_case() drives every fused pass once, on seeded inputs and weights, through
the launch wrappers the learner's update uses (exo_amd/fused.py FusedNets /
FusedTrain: select at 16 and 32 rows per workgroup and its split halves,
target_heads, fixed, encoder, critic phase 0 and phases 1 + 2, actor a / b / c
and the weight-gradient launches they feed) and returns every buffer a pass
writes.  tests/test_fused_core_bits_gpu.py runs the same function and compares
the raw bits with tests/golden/td7f_core_bits.npz, which this script writes:

    python tools/td7f_core_fixture.py            # rewrites the fixture

Generate it at the commit whose arithmetic is the reference (the parent of a
change to the GEMM core that claims bit identity), never at the commit under
test.

Shapes: B = 40 rows (two full 16-row tiles and a ragged one) at
  "default": Hyperparameters() -- 5 tiles per wave; 5, 10, 20 and 30 k-steps
  "w240":    every width 240 -- 4 tiles per wave; the 480-wide concatenated
             input gives 15 k-steps, the 720-wide one 25
for bf16, fp16 and fp32 (fp32 doubles the k-steps).

Storage: arrays of at most WHOLE bytes whole; larger ones as the SHA-256 of
their bytes plus their first 64 elements (key + "#sha" / "#head").
"""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "a-deep-reinforcement-learning-enabled-soft-exoskeleton-for-parkinson-s-patients_amd")
for _p in (PKG, os.path.join(REPO, "tests"), os.path.join(REPO, "oracle"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIXTURE = os.path.join(REPO, "tests", "golden", "td7f_core_bits.npz")
B = 40
SETS = {"default": None, "w240": 240}
PRECISIONS = ("bf16", "fp16", "fp32")
CASES = [(s, p) for s in SETS for p in PRECISIONS]
WHOLE = 2048  # bytes; 64 KiB would put the six cases' fp32 activations (48 KiB each) well past 1 MB
HEAD = 64


def _learner(precision, width):
    """tests/test_fused_train_parity_gpu.py's learner: the seeded CPU initial
    state (target / fixed nets and the actor perturbed), loaded and packed."""
    import torch
    from exo_amd import fused
    from exo_amd.td7 import TD7Learner
    from helpers import TD7_FULL_LEARNING_STEPS
    from td7_restate import NETS, perturbed_cpu_learner, width_hp

    hp = width_hp(width)
    C = perturbed_cpu_learner(hp, (-1.0, 2.0))
    f0 = fused.FUSED_F32
    fused.FUSED_F32 = precision == "fp32"
    try:
        L = TD7Learner(80, 7, hp, learning_steps=TD7_FULL_LEARNING_STEPS, device="cuda", precision=precision)
    finally:
        fused.FUSED_F32 = f0
    for name in NETS:
        getattr(L, name).load_state_dict(getattr(C, name).state_dict())
    L.min_target.fill_(-1.0)
    L.max_target.fill_(2.0)
    L.max.fill_(-1e8)
    L.min.fill_(1e8)
    assert L.fused is not None and L.fused_train, getattr(L.fused, "train_error", "the per-layer kernels run this shape")
    L.fused.pack_all()
    torch.cuda.synchronize()
    return L


def _np(t):
    """raw bits of a device tensor (int16 bit storage stays int16)"""
    return t.detach().contiguous().cpu().numpy().copy()


def _xt(out, key, bufs):
    for i, xb in enumerate(bufs):
        out[f"{key}{i}.x"] = _np(xb.x)
        out[f"{key}{i}.dp"] = _np(xb.dp)
        out[f"{key}{i}.part"] = _np(xb.part)


def run_case(setname, precision):
    """name -> numpy array of every buffer the fused passes write, in a fixed order of launches."""
    import torch
    from td7_restate import td7_batch

    L = _learner(precision, SETS[setname])
    F = L.fused
    s, a, ns, r, nd, z = [torch.tensor(x, device="cuda") for x in td7_batch(B, 0)]
    out = {}
    # select_action: 16 and 32 rows per workgroup, then the split halves (same Philox stream, advancing).
    # Its observations are the first B rows of a buffer of whole 32-row tiles: builds before the
    # row_issue clamp (csrc/td7_fused.h) stage the row after the last 32-row tile's first half
    # unmasked -- B + 8 here, outside a B-row tensor -- and this script must run on them
    obs = torch.zeros((-(-B // 32) * 32, s.shape[1]), device="cuda")
    obs[:B] = s
    obs = obs[:B]
    out["select.rt1"] = _np(F.select(obs, rt=1))
    out["select.rt2"] = _np(F.select(obs, rt=2))
    img = F.select_zs(obs, rt=1)
    out["select.zimg"] = _np(img)
    out["select.zm12"] = _np(F.select(obs, rt=1, zs_img=img))
    out["select.sigma"] = _np(L.exploration_noise_t.reshape(1))
    # the critic target chain (target_a + target_b) and the fixed embeddings
    qt = F.target_heads(ns, noise=z)
    out["target.qt"] = _np(qt)
    out["target.img"] = _np(F._img(B)[:B])
    zs, zsa = F.fixed(s, a)
    out["fixed.zs"], out["fixed.zsa"] = _np(zs), _np(zsa)
    # the gradient passes
    tr = F.train(B)
    tr.encoder(s, a, ns)
    for i, y in enumerate(tr.y_enc):
        out[f"encoder.y{i}"] = _np(y)
    _xt(out, "encoder.xt", tr.xt_enc)
    for tag, phases in (("critic.p0", (0,)), ("critic.p12", (1, 2))):
        for t in (tr.td, tr.q, *tr.y_critic, tr.crit_q, tr.crit_h0, tr.crit_mean):
            t.zero_()
        for xb in tr.xt_critic:
            xb.x.zero_(), xb.dp.zero_(), xb.part.zero_()
        for ph in phases:
            tr.critic(s, a, zs, zsa, qt, r, nd, phase=ph)
        out[f"{tag}.td"], out[f"{tag}.q"] = _np(tr.td), _np(tr.q)
        out[f"{tag}.y1"], out[f"{tag}.y2"] = _np(tr.y_critic[0]), _np(tr.y_critic[1])
        _xt(out, f"{tag}.xt", tr.xt_critic)
    out["critic.p12.h0"] = _np(tr.crit_h0)
    out["critic.minmax"] = np.array([float(L.min), float(L.max)], dtype=np.float32)
    out["wgrad.prio"] = _np(tr.wgrad_encoder_critic())
    out["wgrad.enc"], out["wgrad.critic"] = _np(tr.enc_grad), _np(tr.critic_grad)
    for ph in (0, 1, 2):
        tr.actor(ph, s, zs)
    tr.wgrad_actor()
    for k in ("act_out", "zsa_out", "h0", "mean0", "da", "dzsa"):
        out[f"actor.{k}"] = _np(getattr(tr, k))
    for k in ("ya", "yz", "yc"):
        for i, t in enumerate(getattr(tr, k)):
            out[f"actor.{k}{i}"] = _np(t)
    _xt(out, "actor.xt", tr.xt_actor)
    out["wgrad.actor"] = _np(tr.actor_grad)
    torch.cuda.synchronize()
    return out


def digest(arr):
    """what the fixture keeps of one array: {suffix: array}"""
    arr = np.ascontiguousarray(arr)
    if arr.nbytes <= WHOLE:
        return {"": arr}
    sha = np.frombuffer(hashlib.sha256(arr.tobytes()).digest(), dtype=np.uint8)
    return {"#sha": sha, "#head": arr.reshape(-1)[:HEAD].copy()}


def main():
    store = {}
    for setname, precision in CASES:
        res = run_case(setname, precision)
        for name, arr in res.items():
            assert np.isfinite(arr.astype(np.float64)).all() or arr.dtype == np.int16, name
            for suffix, v in digest(arr).items():
                store[f"{setname}/{precision}/{name}{suffix}"] = v
        print(setname, precision, len(res), "arrays", flush=True)
    np.savez_compressed(FIXTURE, **store)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
