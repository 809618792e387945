"""The coloured-noise generator launch (td7f_pink_advance) alone, at the
Collector's shape: 15 stand-in policies x 800 envs, env i of a segment on
motion i % 8 (sequence lengths 232..347).

--mode all : every env flagged done (the construction-time fill);
--mode few : the typical step -- every env stepped, `--done` random envs
             flagged (default 40: 12,000 envs / ~300 steps per episode), a
             fresh random set per launch.

Prints microseconds per launch from device events around `--launches`
launches; run it under `rocprofv3 --kernel-trace --stats -- python ...` (one
mode per run) for the kernel's own durations.

usage: python tools/pink_generator_bench.py --mode {all,few} [--launches 50] [--done 40]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "a-deep-reinforcement-learning-enabled-soft-exoskeleton-for-parkinson-s-patients_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from exo_amd import _native as nat, motions  # noqa: E402
from exo_amd.fused import PinkNoise, PolicySet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=("all", "few"))
    ap.add_argument("--policies", type=int, default=15)
    ap.add_argument("--envs-per-policy", type=int, default=800)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--done", type=int, default=40)
    a = ap.parse_args()
    from eval_bench import stand_ins
    dev = nat.require_gpu("cuda:0")
    K, per = a.policies, a.envs_per_policy
    n = K * per
    ps = PolicySet(stand_ins(K, dev), "bf16", dev)
    _, lengths = motions.load()
    ln = np.asarray(lengths)[np.tile(np.arange(per) % 8, K)]
    pn = PinkNoise(ps, [per * k for k in range(K + 1)], ln, 0.1)
    ones = torch.ones(n, dtype=torch.bool, device=dev)
    g = torch.Generator().manual_seed(0)
    masks = []
    for _ in range(a.launches):
        if a.mode == "all":
            masks.append(ones)
        else:
            m = torch.zeros(n, dtype=torch.bool)
            m[torch.randperm(n, generator=g)[:a.done]] = True
            masks.append(m.to(dev))
    for m in masks[:3]:  # warm-up
        pn.advance(ones, m)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for m in masks:
        pn.advance(ones, m)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps(dict(mode=a.mode, envs=n, done_per_launch=n if a.mode == "all" else a.done, launches=a.launches,
                          us_per_launch=e0.elapsed_time(e1) * 1e3 / a.launches)))


if __name__ == "__main__":
    main()
