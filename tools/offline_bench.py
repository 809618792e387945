"""ms per exo_amd.OfflineTrainer.step(): offline TD7+BC on a synthetic dataset.

    python tools/offline_bench.py --precision bf16
    EXO_OFFLINE_FUSED=0 python tools/offline_bench.py --precision bf16   # the autograd actor update
    python tools/offline_bench.py --precision bf16 --view 4              # the same dataset as a view of a 4x larger buffer

B = 8 strata x 128 rows, the default widths, a 200k-row dataset (8 x 25,000),
device events around --steps graph-replayed steps after --warmup.  Prints one
JSON line.  A/B: run the two commands as alternating processes, repeated, and
compare the difference with the repeated runs' spread.

--view K: the dataset's rows are source 0 of a tagged buffer that holds K rows
for each of them (row i's copies tagged 1..K-1 follow it), and the agent
trains from LAP.view([0]) through Agent.use_replay -- the same rows in the
same order as the compact load, in a tree over K times the slots."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "a-deep-reinforcement-learning-enabled-soft-exoskeleton-for-parkinson-s-patients_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--strata", type=int, default=8)
    ap.add_argument("--batch", type=int, default=128, help="rows per stratum")
    ap.add_argument("--lmbda", type=float, default=0.1)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--view", type=int, default=0, help="K: train from a view of a K times larger tagged buffer")
    a = ap.parse_args()
    from exo_amd import OfflineTrainer
    from exo_amd import td7
    torch.manual_seed(0)
    hp = td7.Hyperparameters(batch_size=a.batch, lmbda=a.lmbda)
    per = a.rows // a.strata
    ag = td7.Agent(80, 7, 1, offline=True, hp=hp, env_num=a.strata, buffer_size=1 if a.view else per,
                   precision=a.precision, graph_safe=True)
    rng = np.random.default_rng(0)
    n = per * a.strata
    s = rng.normal(0, 1, (n, 80)).astype(np.float32)
    d = dict(state=s, action=rng.uniform(-1, 1, (n, 7)).astype(np.float32),
             next_state=(s + 0.1 * rng.normal(0, 1, (n, 80))).astype(np.float32),
             reward=rng.uniform(-2, 3, n).astype(np.float32), done=rng.uniform(0, 1, n) < 0.02,
             strata=np.tile(np.arange(a.strata, dtype=np.int32), per))
    if a.view:
        from exo_amd.replay import LAP
        base = LAP(80, 7, ag.device, a.strata, max_size=per * a.view, batch_size=a.batch)
        base.load_dataset(**{k: np.repeat(v, a.view, axis=0) for k, v in d.items()},
                          source=np.tile(np.arange(a.view, dtype=np.int32), n))
        ag.use_replay(base.view([0]))
    else:
        ag.replay_buffer.load_dataset(**d)
    t = OfflineTrainer(ag, use_graphs=not a.eager)
    t.run(a.warmup)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t.run(a.steps)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    L = ag.learner
    finite = all(bool(torch.isfinite(p).all()) for p in L.actor.parameters())
    print(json.dumps(dict(metric="offline_ms_per_step", ms_per_step=round(ms, 5), precision=a.precision,
                          rows=a.strata * a.batch, dataset_rows=n, view=a.view, steps=a.steps, warmup=a.warmup,
                          graphs=not a.eager, fused_train=bool(L.fused_train), offline_fused=bool(td7.OFFLINE_FUSED),
                          lmbda=a.lmbda, training_steps=L.training_steps, finite=finite)))
    t.release_graphs()


if __name__ == "__main__":
    main()
