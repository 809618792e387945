"""Collector(tag_sources=True): 3 seeded stand-in policies x 8 envs, 40 steps,
eager and graph=True.  The replay's source column counts, per policy, the
transitions report() gives; no row is untagged; and a twin collector without
the flag fills an identical buffer (rows, tree, ring state)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K, N, STEPS = 3, 8, 40
ROWS = ("state", "action", "next_state", "reward", "not_done")
SEQS = ([1, 0, 1, 0, 0, 0, 0], [0, 1, 1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0])


def _stand_ins():
    from exo_amd.td7 import Actor, Encoder, Hyperparameters
    hp = Hyperparameters()
    out = []
    for k in range(K):
        torch.manual_seed(1000 + k)
        out.append((Actor(80, 7, hp.zs_dim, hp.actor_hdim, hp.actor_activ).to("cuda").eval(),
                    Encoder(80, 7, hp.zs_dim, hp.enc_hdim, hp.enc_activ).to("cuda").eval()))
    return out


def _collect(graph, tag):
    from exo_amd import Collector
    from exo_amd.fused import PolicySet
    from exo_amd.replay import LAP
    rb = LAP(80, 7, "cuda", num_envs=8, max_size=256, batch_size=4)
    torch.manual_seed(77)  # the noise streams are keyed by torch's seed
    col = Collector(PolicySet(_stand_ins(), "bf16", torch.device("cuda", 0), None), N, rb, sigma=0.1,
                    per_policy_env_kwargs=[dict(tremor_sequence=np.array(s, dtype=np.float64)) for s in SEQS], seed=5,
                    graph=graph, tag_sources=tag)
    try:
        rep = col.collect(STEPS)
        torch.cuda.synchronize()
        if graph:
            assert len(col._graphs) == 2
    finally:
        col.close()
    return rb, rep


@pytest.mark.parametrize("graph", [False, True])
def test_tagged_collection_counts_every_policy_and_changes_no_row(graph):
    rb, rep = _collect(graph, True)
    twin, _ = _collect(graph, False)
    assert twin.source is None and rb.source is not None
    counts = rb.source_counts(K).cpu().numpy()
    assert counts[:, K].sum() == 0
    assert counts[:, :K].sum(0).tolist() == [r["transitions"] for r in rep] == [N * STEPS] * K
    assert int(rb.size_s.sum()) == K * N * STEPS  # nothing wrapped: every transition is counted
    for name in ROWS:
        assert torch.equal(getattr(rb, name)[:, :256], getattr(twin, name)[:, :256]), name
    assert torch.equal(rb._tree, twin._tree) and torch.equal(rb.ptr_s, twin.ptr_s)
    assert torch.equal(rb.size_s, twin.size_s) and torch.equal(rb._maxp, twin._maxp)
    # env i of a segment runs motion i % 8 = its stratum: every stratum holds STEPS rows of every policy
    assert (counts[:, :K] == STEPS).all()
    v = rb.view([1])
    assert torch.equal(v.totals, torch.full((8,), float(STEPS), device="cuda"))
