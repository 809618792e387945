"""Growing-batch training from one shared collection: K stand-in behaviour
policies fill one replay (Collector, tag_sources=True) and K offline agents
each train on their own policy's rows through replay.view([p], live=True),
in rounds of collect(c) steps then m training steps per agent.  The views
follow the inserts (lap_views_follow), so the agents keep the priorities they
have learned and see their policy's new rows, through ring wraps too.

    python tools/growing_batch.py --policies 4 --envs-per-policy 64 --rounds 6 --collect 40 --train 50

Per round: the transitions collected so far, every view's kept rows (summed
over the strata), the trainers' resamples so far, and ms per collect step and
per training step (host clock around a device synchronise).  Prints one JSON
line at the end."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "a-deep-reinforcement-learning-enabled-soft-exoskeleton-for-parkinson-s-patients_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=4)
    ap.add_argument("--envs-per-policy", type=int, default=64)
    ap.add_argument("--capacity", type=int, default=2000, help="replay slots per stratum (small: the rings wrap)")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--collect", type=int, default=40, help="collector steps per round")
    ap.add_argument("--train", type=int, default=50, help="training steps per agent and round")
    ap.add_argument("--batch-size", type=int, default=32, help="rows per stratum and training step")
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp16", "fp32"))
    ap.add_argument("--eager", action="store_true", help="no graphs (collector and trainers)")
    a = ap.parse_args()
    from eval_bench import CONFIGS, stand_ins
    from exo_amd import Collector, OfflineTrainer
    from exo_amd import _native as nat
    from exo_amd.fused import PolicySet
    from exo_amd.replay import LAP
    from exo_amd.td7 import Agent, Hyperparameters
    dev = nat.require_gpu("cuda:0")
    K, n = a.policies, a.envs_per_policy
    rb = LAP(80, 7, dev, 8, max_size=a.capacity, batch_size=a.batch_size)
    col = Collector(PolicySet(stand_ins(K, dev), a.precision, dev, None), [n] * K, rb, sigma=0.1,
                    per_policy_env_kwargs=[dict(tremor_sequence=CONFIGS[k % 15]) for k in range(K)],
                    graph=not a.eager, tag_sources=True)
    views = [rb.view([p], live=True) for p in range(K)]
    agents, trainers, rounds = [], [], []
    for r in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        col.collect(a.collect)
        torch.cuda.synchronize()
        t_col = (time.perf_counter() - t0) * 1e3 / a.collect
        if not trainers:  # the first rows are there: the agents on their views
            for p, v in enumerate(views):
                torch.manual_seed(100 + p)
                ag = Agent(80, 7, 1, offline=True, hp=Hyperparameters(batch_size=a.batch_size), env_num=8, device=dev,
                           buffer_size=1, precision=a.precision, graph_safe=True)
                ag.use_replay(v)
                agents.append(ag)
                trainers.append(OfflineTrainer(ag, use_graphs=not a.eager))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in trainers:
            t.run(a.train)
        torch.cuda.synchronize()
        t_train = (time.perf_counter() - t0) * 1e3 / (a.train * K)
        row = dict(round=r + 1, transitions=K * n * col.steps_run, kept=[int(v.kept.sum()) for v in views],
                   resamples=[t.resamples for t in trainers], collect_ms_per_step=round(t_col, 4),
                   train_ms_per_step=round(t_train, 4))
        rounds.append(row)
        print(f"round {row['round']:3d}  transitions {row['transitions']:9d}  kept {row['kept']}  "
              f"resamples {row['resamples']}  collect {t_col:.3f} ms/step  train {t_train:.3f} ms/step", flush=True)
    # every view holds exactly its policy's stored rows, and only those have a priority
    counts = rb.source_counts(K)[:, :K].cpu()
    for p, v in enumerate(views):
        assert v.kept.cpu().tolist() == counts[:, p].tolist(), p
        assert torch.equal(v.priority > 0, rb.source[:, :a.capacity] == p), p
    for t in trainers:
        t.release_graphs()
    col.close()
    print(json.dumps(dict(metric="growing_batch", policies=K, envs_per_policy=n, capacity=a.capacity,
                          precision=a.precision, graphs=not a.eager, rounds=rounds)))


if __name__ == "__main__":
    main()
