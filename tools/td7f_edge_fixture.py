"""Bit fixture of the fused TD7 gradient passes at the edges of their VALU
stretches (csrc/td7_fused.h norm_bwd / make_dp, the Q head's rank-1 dX, the
loss block of td7f_critic, the tanh' block of td7f_actor phase 2).

Sibling of tools/td7f_core_fixture.py (whose learner it shares);
tests/test_fused_edge_bits_gpu.py runs run_case() and compares the raw bits
with tests/golden/td7f_edge_bits.npz, which this script writes:

    python tools/td7f_edge_fixture.py            # rewrites the fixture

Generate it with the library of the commit whose arithmetic is the reference
(EXO_AMD_LIB names a library file beside the product one), never with the
build under test.

Cases: {default widths (5 tiles per wave), every width 240 (4 tiles)} x
{bf16, fp16, fp32} x B in
  1   one live row, 15 padded
  17  a second row tile with one live row, and in the first tile:
      rows ZERO = (3, 7): state and action zero, q0's and the actor's l0 bias
          zeroed, so q0 / l0's pre-norm output is exactly zero -- the
          m < eps arm of norm_bwd in critic, actor phase 1 (its action row
          zeroed after phase 0) and actor phase 2
      row TD0 = 5: reward = Q of head 0 from a first forward, not_done = 0:
          TD error exactly 0 for head 0, dq = +-0 through the rank-1 path
      "critic.tiny": a further critic pass with q1 / q2 / q3's biases zeroed
          too and zero embeddings on the ZERO rows, so their Q is exactly 0,
          and reward 3e-38 on row 7: |d| = 3e-38, dq = d / 17 subnormal in
          fp32 and bf16, zero in fp16

Not every recorded value is finite: on a ZERO row the m < eps arm gives
gx = dy / 1e-8, which x 2^10 is past fp16's range, so the fp16 cases at B = 17
carry inf / nan from there on (into the weight gradients too).  The fixture
keeps the reference's bits as they are.

Storage: per case the sorted array names and one SHA-256 each over the
array's dtype, shape and bytes (12 cases x ~180 arrays: heads or whole arrays
as in the core fixture would pass the 1 MiB a committed file may take).
"""
import hashlib
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("td7f_core_fixture", os.path.join(REPO, "tools", "td7f_core_fixture.py"))
core = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(core)

FIXTURE = os.path.join(REPO, "tests", "golden", "td7f_edge_bits.npz")
SETS = core.SETS
PRECISIONS = core.PRECISIONS
BATCHES = (1, 17)
CASES = [(s, p, b) for s in SETS for p in PRECISIONS for b in BATCHES]
ZERO = (3, 7)
TD0 = 5
TINY = 3e-38
_np, _xt = core._np, core._xt


def _critic(out, tag, tr, args, phases):
    for t in (tr.td, tr.q, *tr.y_critic, tr.crit_q, tr.crit_h0, tr.crit_mean):
        t.zero_()
    for xb in tr.xt_critic:
        xb.x.zero_(), xb.dp.zero_(), xb.part.zero_()
    for ph in phases:
        tr.critic(*args, phase=ph)
    out[f"{tag}.td"], out[f"{tag}.q"] = _np(tr.td), _np(tr.q)
    out[f"{tag}.y1"], out[f"{tag}.y2"] = _np(tr.y_critic[0]), _np(tr.y_critic[1])
    _xt(out, f"{tag}.xt", tr.xt_critic)


def _actor(out, tag, tr):
    for k in ("act_out", "zsa_out", "h0", "mean0", "da", "dzsa"):
        out[f"{tag}.{k}"] = _np(getattr(tr, k))
    for k in ("ya", "yz", "yc"):
        for i, t in enumerate(getattr(tr, k)):
            out[f"{tag}.{k}{i}"] = _np(t)
    _xt(out, f"{tag}.xt", tr.xt_actor)


def run_case(setname, precision, B):
    """name -> numpy array of every buffer the gradient passes write, in a fixed order of launches."""
    import torch
    from td7_restate import td7_batch

    L = core._learner(precision, SETS[setname])
    F = L.fused
    edges = B > max(ZERO + (TD0,))
    with torch.no_grad():
        L.critic.b0.zero_()
        L.actor.l0.bias.zero_()
    s, a, ns, r, nd, z = [torch.tensor(x, device="cuda") for x in td7_batch(B, 0)]
    if edges:
        s[list(ZERO)] = 0.0
        a[list(ZERO)] = 0.0
    out = {}
    qt = F.target_heads(ns, noise=z)
    zs, zsa = F.fixed(s, a)
    tr = F.train(B)
    tr.encoder(s, a, ns)
    for i, y in enumerate(tr.y_enc):
        out[f"encoder.y{i}"] = _np(y)
    _xt(out, "encoder.xt", tr.xt_enc)
    if edges:  # TD error exactly zero for head 0 of row TD0
        tr.critic(s, a, zs, zsa, qt, r, nd, phase=0)
        r[TD0, 0] = tr.q[TD0, 0]
        nd[TD0, 0] = 0.0
    _critic(out, "critic.p0", tr, (s, a, zs, zsa, qt, r, nd), (0,))
    if edges:
        assert out["critic.p0.td"][TD0, 0] == 0.0
    _critic(out, "critic.p12", tr, (s, a, zs, zsa, qt, r, nd), (1, 2))
    out["critic.p12.h0"] = _np(tr.crit_h0)
    out["critic.p12.mean"] = _np(tr.crit_mean)
    if edges:
        assert (out["critic.p12.mean"].reshape(2, -1)[:, list(ZERO)] == 0).all(), "q0's output is not zero on the ZERO rows"
    out["critic.minmax"] = np.array([float(L.min), float(L.max)], dtype=np.float32)
    out["wgrad.prio"] = _np(tr.wgrad_encoder_critic())
    out["wgrad.enc"], out["wgrad.critic"] = _np(tr.enc_grad), _np(tr.critic_grad)
    # the actor passes; phase 1's action row is zeroed on the ZERO rows (its q0 sees [0, 0])
    tr.actor(0, s, zs)
    _actor(out, "actor.a", tr)
    if edges:
        assert (tr.mean0[list(ZERO)] == 0).all(), "l0's output is not zero on the ZERO rows"
        tr.act_out[list(ZERO)] = 0.0
    tr.actor(1, s, zs)
    tr.actor(2, s, zs)
    tr.wgrad_actor()
    _actor(out, "actor", tr)
    out["wgrad.actor"] = _np(tr.actor_grad)
    # the offline update's phases with the TD3+BC term
    tr.actor(1, s, zs, action=a, lmbda=0.1)
    tr.actor(2, s, zs, action=a, lmbda=0.1)
    _actor(out, "actor.bc", tr)
    out["actor.bc.qabs"] = _np(tr.qabs)
    if edges:  # Q exactly zero on the ZERO rows, |d| = TINY on the second
        with torch.no_grad():
            for k in (1, 2, 3):
                getattr(L.critic, f"b{k}").zero_()
        zs2, zsa2 = zs.clone(), zsa.clone()
        zs2[list(ZERO)] = 0.0
        zsa2[list(ZERO)] = 0.0
        r[list(ZERO), 0] = torch.tensor([0.25, TINY], device="cuda")
        nd[list(ZERO), 0] = 0.0
        _critic(out, "critic.tiny", tr, (s, a, zs2, zsa2, qt, r, nd), (0,))
        if os.environ.get("TD7F_EDGE_VERBOSE"):  # expected: Q 0 on the ZERO rows, |td| TINY on the second
            print("  tiny: q", out["critic.tiny.q"][list(ZERO)].tolist(), "td", out["critic.tiny.td"][list(ZERO)].tolist())
    torch.cuda.synchronize()
    return out


def digest(arr):
    """SHA-256 over dtype, shape and bytes, as 32 uint8"""
    arr = np.ascontiguousarray(arr)
    h = hashlib.sha256(f"{arr.dtype.str}{arr.shape}".encode())
    h.update(arr.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def digests(res):
    """(sorted names [n], digests [n, 32]) of a run_case result"""
    names = sorted(res)
    return np.array(names), np.stack([digest(res[k]) for k in names])


def main():
    store = {}
    for setname, precision, B in CASES:
        res = run_case(setname, precision, B)
        key = f"{setname}/{precision}/{B}"
        store[key + "/names"], store[key + "/sha"] = digests(res)
        print(setname, precision, B, len(res), "arrays", flush=True)
    np.savez_compressed(FIXTURE, **store)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
