"""lap_update_sample's sibling-chain kernel (csrc/lap.hip,
lap_update_sample_chain_kernel: the global levels of the priority update as
one round trip plus LDS work) against the two launches it replaces,
LAP.update_priority then LAP.sample, on a twin buffer: every tree node,
max_priority, the sampled indices, the gathered rows and the RNG call counter
bit for bit, over 4 consecutive calls so the tree evolves.

Shapes: no global level (40 slots), exactly one (cap 8,192), two, the bench's
depth (6), one draw, and 1,024 draws (above the chain's batch bound: the level-
sweep kernel).  Index patterns (tests/lap_chain_cases.py): the collisions the
chain resolves through its partner table, each at the full sampling size and
at a size below the capacity (the prefix-total path)."""
import functools

import numpy as np
import pytest
import torch

from lap_chain_cases import global_levels, pattern, pattern_names

pytestmark = pytest.mark.gpu

SHAPES = [(8, 40, 16), (8, 5_000, 128), (3, 12_000, 64), (8, 250_000, 128), (1, 250_000, 1), (2, 30_000, 1024)]
ROWS = ("state", "action", "next_state", "reward", "not_done")


def _cap(C):
    cap = 1
    while cap < C:
        cap <<= 1
    return cap


@functools.lru_cache(maxsize=1)
def _twins(E, C, B):
    """Two buffers with the same rows, and the tree of the same non-integer
    priorities (built once per shape; every test starts from a copy)."""
    from exo_amd.replay import LAP
    a, b = (LAP(80, 7, "cuda", E, max_size=C, batch_size=B) for _ in range(2))
    g = torch.Generator(device="cuda").manual_seed(5)
    for name in ROWS:
        getattr(a, name).normal_(generator=g)
        getattr(b, name).copy_(getattr(a, name))
    cap = a._cap
    assert cap == _cap(C)
    prio = np.zeros((E, cap), dtype=np.float32)
    prio[:, :C] = np.random.default_rng(C + B).gamma(0.7, 2.0, (E, C)).astype(np.float32) + np.float32(1e-3)
    tree = torch.zeros((E, 2 * cap), dtype=torch.float32, device="cuda")
    tree[:, cap:] = torch.as_tensor(prio, device="cuda")
    n = cap
    while n > 1:  # every node exactly left + right
        tree[:, n // 2:n] = tree[:, n:2 * n:2] + tree[:, n + 1:2 * n:2]
        n //= 2
    return a, b, tree


def _start(E, C, B, size):
    a, b, tree = _twins(E, C, B)
    for lap in (a, b):
        lap._tree.copy_(tree)
        lap._maxp.fill_(1.0)
        lap.size_s.fill_(size)
        lap._rng.state.zero_()
        lap.fuse_update_sample = True
    return a, b


def _same(a, b, ba, bb, tag):
    torch.cuda.synchronize()
    assert torch.equal(b._tree, a._tree), tag
    assert float(a._maxp) == float(b._maxp), tag
    assert torch.equal(a.ind, b.ind), tag
    for x, y in zip(ba, bb):
        assert torch.equal(x, y), tag
    assert torch.equal(a._rng.state, b._rng.state), tag


def _indices(name, rng, E, B, size):
    return np.stack([pattern(name, rng, B, size) for _ in range(E)])


CASES = [(E, C, B, below, name) for (E, C, B) in SHAPES for below in (False, True) for name in pattern_names(_cap(C))]


@pytest.mark.parametrize("E,C,B,below,name", CASES)
def test_chain_update_and_sample_equals_the_two_launches(E, C, B, below, name):
    size = (C * 7) // 10 + 1 if below else C
    a, b = _start(E, C, B, size)
    rng = np.random.default_rng([C, B, size])
    for it in range(4):
        ind = torch.as_tensor(_indices(name, rng, E, B, size), device="cuda")
        p = torch.as_tensor(rng.uniform(0.1, 9.0, E * B).astype(np.float32), device="cuda")
        a.update_priority(p, ind)
        ba = a.sample(it % 2)
        bb = b.update_priority_and_sample(p, ind, it % 2)
        _same(a, b, ba, bb, (name, it))


@pytest.mark.parametrize("E,C,B", SHAPES)
def test_indices_then_rows_form_equals_the_two_launches(E, C, B):
    """before_gather=: lap_update_sample_idx, then lap_gather_rows."""
    size = C - 1
    a, b = _start(E, C, B, size)
    rng = np.random.default_rng(B)
    called = []
    for it in range(4):
        ind = torch.as_tensor(_indices("dups" if it % 2 else "one_block", rng, E, B, size), device="cuda")
        p = torch.as_tensor(rng.uniform(0.1, 9.0, E * B).astype(np.float32), device="cuda")
        a.update_priority(p, ind)
        ba = a.sample(it % 2)
        bb = b.update_priority_and_sample(p, ind, it % 2, before_gather=lambda: called.append(it))
        _same(a, b, ba, bb, it)
    assert called == [0, 1, 2, 3]


def test_the_sampled_indices_may_be_updated_in_place():
    """The caller's previous batch in the same slot: idx_in is idx_out."""
    E, C, B = 8, 250_000, 128
    a, b = _start(E, C, B, 180_001)
    rng = np.random.default_rng(2)
    a.sample(0)
    b.sample(0)
    for it in range(4):
        p = torch.as_tensor(rng.uniform(0.1, 9.0, E * B).astype(np.float32), device="cuda")
        a.update_priority(p)          # a.ind: the batch just sampled
        ba = a.sample(0)
        bb = b.update_priority_and_sample(p, None, 0)
        _same(a, b, ba, bb, it)


def test_td_form_equals_the_level_sweep_kernel_and_the_two_launches(monkeypatch):
    """lap_update_sample_td: the priorities computed in the launch from |td|.
    The chain against EXO_LAP_CHAIN=0 (the same launch on the level-sweep
    kernel: priorities included), and against update_priority(those
    priorities) + sample."""
    E, C, B = 8, 250_000, 128
    size = 176_128
    runs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("EXO_LAP_CHAIN", flag)
        a, b = _start(E, C, B, size)
        prng = np.random.default_rng(12)
        out = []
        for it in range(4):
            ind = torch.as_tensor(_indices("dups" if it % 2 else "pairs_xor1", prng, E, B, size), device="cuda")
            td = torch.as_tensor(prng.gamma(0.7, 1.0, (E * B, 2)).astype(np.float32), device="cuda")
            pr = torch.empty(E * B, device="cuda")
            bb = b.update_priority_and_sample_td(td, 0.4, 1.0, ind, it % 2, prio_out=pr)
            a.update_priority(pr, ind)
            ba = a.sample(it % 2)
            _same(a, b, ba, bb, (flag, it))
            out.append((pr.clone(), b._tree.clone(), b.ind.clone()))
        runs.append(out)
    for x, y in zip(*runs):
        for u, v in zip(x, y):
            assert torch.equal(u, v)


def test_flag_restores_the_level_sweep_kernel(monkeypatch):
    """EXO_LAP_CHAIN=0: lap_update_sample_kernel, the same results."""
    monkeypatch.setenv("EXO_LAP_CHAIN", "0")
    E, C, B = 8, 250_000, 128
    size = 180_001
    a, b = _start(E, C, B, size)
    rng = np.random.default_rng(4)
    for it in range(4):
        ind = torch.as_tensor(_indices("dups", rng, E, B, size), device="cuda")
        p = torch.as_tensor(rng.uniform(0.1, 9.0, E * B).astype(np.float32), device="cuda")
        a.update_priority(p, ind)
        ba = a.sample(it % 2)
        bb = b.update_priority_and_sample(p, ind, it % 2)
        _same(a, b, ba, bb, it)


def test_td_form_in_the_trainer_does_not_change_training(monkeypatch):
    """The graph-replayed trainer with the update forked after the critic pass
    (lap_update_sample_td, as tests/test_trainer_fusion_gpu.py builds it): the
    chain against EXO_LAP_CHAIN=0 -- the same weights and replay tree."""
    import exo_amd.rollout as rollout
    from test_trainer_fusion_gpu import _assert_same, _make, _params
    monkeypatch.setattr(rollout.VecTrainer, "us_after_critic", True)
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("EXO_LAP_CHAIN", flag)
        t, ag = _make(seed=9)
        for _ in range(10):
            t.step()
        torch.cuda.synchronize()
        outs.append((_params(ag), ag.replay_buffer._tree.clone()))
    _assert_same(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


def test_shapes_cover_every_count_of_global_levels():
    assert [global_levels(_cap(C)) for _, C, _ in SHAPES] == [0, 1, 2, 6, 6, 3]
