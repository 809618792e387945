"""Live views under Collector and OfflineTrainer: 2 seeded stand-in policies x 8
envs tagged into a replay of 8 strata x 23 slots.  Every step puts one row of
each policy into every stratum, so policy 0 owns the even slots until the ring
(23 slots: odd) wraps, then the odd ones: a view that did not follow would hold
foreign rows after the first wrap.

* graph=True: the follow launch is recorded with the step.  The views' trees
  and kept equal an eager twin's bit for bit, and attaching a third view makes
  the next collect() record its graphs again.
* An offline agent on view [0] alternates with the collector: the trainer
  draws its pending batch again once (resamples), never trains on a foreign
  row, and the view's tree stays a sum tree over policy 0's rows alone."""
import numpy as np
import pytest
import torch

from lap_view_model import build_tree, cap_of

pytestmark = pytest.mark.gpu

K, N, E, C = 2, 8, 8, 23
SEQS = ([1, 0, 1, 0, 0, 0, 0], [0, 1, 1, 1, 0, 0, 0])


def _stand_ins():
    from exo_amd.td7 import Actor, Encoder, Hyperparameters
    hp = Hyperparameters()
    out = []
    for k in range(K):
        torch.manual_seed(1000 + k)
        out.append((Actor(80, 7, hp.zs_dim, hp.actor_hdim, hp.actor_activ).to("cuda").eval(),
                    Encoder(80, 7, hp.zs_dim, hp.enc_hdim, hp.enc_activ).to("cuda").eval()))
    return out


def _collector(graph):
    from exo_amd import Collector
    from exo_amd.fused import PolicySet
    from exo_amd.replay import LAP
    rb = LAP(80, 7, "cuda", num_envs=E, max_size=C, batch_size=4)
    torch.manual_seed(77)  # the noise streams are keyed by torch's seed
    col = Collector(PolicySet(_stand_ins(), "bf16", torch.device("cuda", 0), None), N, rb, sigma=0.1,
                    per_policy_env_kwargs=[dict(tremor_sequence=np.array(s, dtype=np.float64)) for s in SEQS], seed=5,
                    graph=graph, tag_sources=True)
    return rb, col


def _state(rb, views):
    torch.cuda.synchronize()
    for v in views:  # kept is the number of the view's sources among the stored rows
        mine = torch.isin(rb.source[:, :C], torch.tensor(v.keep, device="cuda", dtype=torch.int32))
        assert torch.equal(v.kept.long(), mine.sum(1))
        assert torch.equal(v.priority > 0, mine)
    return ([v._tree.clone() for v in views], [v.kept.clone() for v in views], rb._tree.clone(), rb.source.clone(),
            rb.ptr_s.clone())


def _run(graph):
    rb, col = _collector(graph)
    try:
        views = [rb.view([0], live=True), rb.view([1], live=True)]
        col.collect(30)
        first = _state(rb, views)
        recorded = dict(col._graphs)
        assert len(recorded) == (2 if graph else 0)
        views.append(rb.view([0, 1], live=True))
        col.collect(6)
        second = _state(rb, views)
        if graph:  # recorded again, for three views
            assert len(col._graphs) == 2 and col._live_gen == rb.live_generation == 3
            assert all(col._graphs[c] is not recorded[c] for c in (0, 1))
        assert rb.insert_epoch >= 36 and int(rb.size_s.min()) == C  # 72 rows per stratum: wrapped three times
    finally:
        col.close()
    return first, second


def test_graphed_collection_with_live_views_equals_the_eager_twin():
    got, want = _run(True), _run(False)
    for stage, (g, w) in enumerate(zip(got, want)):
        for part, (a, b) in enumerate(zip(g, w)):
            for x, y in zip(a, b) if isinstance(a, list) else [(a, b)]:
                assert torch.equal(x, y), (stage, part)
    # the full view's tree is the base's: every row is tagged and enters at priority 1
    assert torch.equal(got[1][0][2], got[1][2])


def test_an_offline_agent_follows_its_policy_through_the_wrap():
    from exo_amd import OfflineTrainer
    from exo_amd.td7 import Agent, Hyperparameters
    rb, col = _collector(True)
    try:
        view = rb.view([0], live=True)
        torch.manual_seed(21)
        ag = Agent(80, 7, 1, offline=True, hp=Hyperparameters(batch_size=4, target_update_rate=4), env_num=E,
                   buffer_size=1, precision="bf16", graph_safe=True)
        ag.use_replay(view)
        with pytest.raises(ValueError, match="keeps no row"):
            OfflineTrainer(ag, use_graphs=True)
        col.collect(4)  # 8 of 23 slots per stratum
        t = OfflineTrainer(ag, use_graphs=True)
        rows = torch.arange(E, device="cuda")[:, None]

        def steps(n):
            for _ in range(n):
                t.step()
                kept = rb.source[:, :C] == 0
                for slot in (0, 1):
                    assert bool(kept[rows, view._slot(slot)[1].long()].all())

        steps(4)
        assert t.resamples == 0 and not view.stale
        col.collect(14)  # 36 rows per stratum: the ring wrapped, policy 0 moved to the odd slots
        assert view.stale
        steps(4)
        assert t.resamples == 1 and t.graphs and ag.learner.training_steps == 8
        t.release_graphs()
        torch.cuda.synchronize()
        kept = (rb.source[:, :C] == 0).cpu().numpy()
        assert kept[:, 1::2][:, :6].all() and kept[:, 14::2].all()  # both parities hold policy 0's rows
        leaves = view.priority.cpu().numpy()
        # (the env's rewards keep |td| below min_priority here: a kept leaf may well still be 1)
        assert not leaves[~kept].any() and (leaves[kept] > 0).all()
        tree = view._tree.cpu().numpy()
        for s in range(E):
            assert np.array_equal(tree[s], build_tree(leaves[s], cap_of(C))), s
        assert view.kept.cpu().tolist() == kept.sum(1).tolist()
    finally:
        col.close()
