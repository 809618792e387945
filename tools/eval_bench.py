"""Batched policy evaluation against what it replaces, on one MI355X.

Arm (a), the acting launch alone, K x n rows (default 15 x 800), default
widths, per precision (bf16, fp32); ms per set of K policies' actions:
  multi    one td7f_select_multi launch (exo_amd.fused.PolicySet.act)
  single   K back-to-back td7f_select launches of n rows (16-row tiles, sigma
           = 0: what fused.select issues), one per policy
  torch    K torch-module forwards actor(obs, enc.zs(obs)).clamp(-1, 1), what
           tools/eval_policies.py does per configuration
Arm (b), a whole evaluation of K policies x n envs for one episode; seconds:
  batched  exo_amd.Evaluator (one env of K x n envs, step graph on / off)
  loop     tools/eval_policies.py's loop, one configuration after another
           (an env of n envs and torch modules each), same policies and seeds
The shipped policies are not needed: the policies are seeded stand-ins (the
networks' seeded init), each with its own tremor sequence.

Every arm is warmed up first; the arms alternate inside each repeat, in one
process; times are device events (a) / a host clock around a device
synchronise (b).  Prints min / median / max over the repeats and one JSON line.

usage: python tools/eval_bench.py [--policies 15] [--envs 800] [--repeats 20] [--iters 50]
                                  [--eval-repeats 2] [--arms ab] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "a-deep-reinforcement-learning-enabled-soft-exoskeleton-for-parkinson-s-patients_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from exo_amd import Evaluator, VecExoskeletonEnv  # noqa: E402
from exo_amd import _native as nat  # noqa: E402
from exo_amd import ops  # noqa: E402
from exo_amd.fused import PolicySet, TD7FLin, TD7FNoise  # noqa: E402
from exo_amd.td7 import Actor, Encoder, Hyperparameters  # noqa: E402

CONFIGS = [[(k >> 3) & 1, (k >> 2) & 1, (k >> 1) & 1, k & 1, 0, 0, 0] for k in range(1, 16)]  # the 15 shipped ones


def stand_ins(K, device):
    hp = Hyperparameters()
    out = []
    for k in range(K):
        torch.manual_seed(1000 + k)
        out.append((Actor(80, 7, hp.zs_dim, hp.actor_hdim, hp.actor_activ).to(device).eval(),
                    Encoder(80, 7, hp.zs_dim, hp.enc_hdim, hp.enc_activ).to(device).eval()))
    return out


def stats(xs):
    xs = sorted(xs)
    return dict(min=xs[0], median=xs[len(xs) // 2], max=xs[-1], n=len(xs))


def timed(fn, iters):
    """ms per call of fn over `iters` calls, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


@torch.no_grad()
def arm_a(precision, K, n, repeats, iters, device):
    pols = stand_ins(K, device)
    ps = PolicySet(pols, precision, device)
    seg = [n * k for k in range(K + 1)]
    obs = torch.randn((K * n, 80), device=device, generator=torch.Generator(device=device).manual_seed(1))
    out = torch.empty((K * n, 7), device=device)
    parts = [obs[n * k:n * (k + 1)] for k in range(K)]
    outs = [out[n * k:n * (k + 1)] for k in range(K)]
    rng = ops.DeviceRNG(device, 7)
    sigma = torch.zeros((), dtype=torch.float32, device=device)
    nz = TD7FNoise(rng.seed, rng.tag, 0, rng.counter_ptr, rng.ticket_ptr, sigma.data_ptr(), 0.0, 0.0, 1.0, 0, None, None)
    encs = [(TD7FLin * 3)(*[pl.lin for pl in net.layers[:3]]) for net in ps.nets]
    acts = [(TD7FLin * 4)(*[pl.lin for pl in net.layers[3:]]) for net in ps.nets]
    lib, st = nat.lib(), nat.stream_ptr(device)

    def multi():
        ps.act(obs, seg, out=out)

    def single():
        for k in range(K):
            nat.check(lib.td7f_select(ps.prec, ps.act_codes, encs[k], acts[k], nat.ptr(parts[k]), n, ctypes.byref(nz),
                                      nat.ptr(outs[k]), 0, 1, st), "td7f_select")

    def module():
        for k, (actor, enc) in enumerate(pols):
            actor(parts[k], enc.zs(parts[k])).clamp(-1, 1)
    # the two kernels agree bit for bit (sigma = 0) before anything is timed
    multi()
    want = out.clone()
    out.zero_()
    single()
    torch.cuda.synchronize()
    assert torch.equal(out, want), "td7f_select_multi and td7f_select disagree"
    arms = dict(multi=multi, single=single, torch=module)
    for fn in arms.values():
        timed(fn, max(iters // 5, 3))
    res = {k: [] for k in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            res[name].append(timed(fn, iters))
    return {k: stats(v) for k, v in res.items()}


@torch.no_grad()
def loop_eval(pols, n, seed, device):
    """tools/eval_policies.py evaluate(), the modules given instead of loaded"""
    steps = 0
    for k, (actor, enc) in enumerate(pols):
        env = VecExoskeletonEnv(n, seed=seed, device=device, tremor_sequence=CONFIGS[k % 15])
        obs = env.reset()
        out = env.new_outputs(True)
        counters = torch.zeros((n, 5), dtype=torch.float32, device=device)
        done = out[2]
        st = torch.zeros(n, dtype=torch.float32, device=device)
        for _ in range(env.max_len):
            active = done == 0
            a = actor(obs, enc.zs(obs)).clamp(-1, 1)
            obs, _, _, info = env.step(a, active=active, out=out)
            counters = env.eval_metrics(info, stepped=active, counters=counters)
            st += active.float()
        assert bool(done.bool().all())
        steps += int(st.sum().item())
        env.close()
    return steps


def arm_b(K, n, repeats, device):
    pols = stand_ins(K, device)
    per = [dict(tremor_sequence=CONFIGS[k % 15]) for k in range(K)]
    res = {"batched_graph": [], "batched_eager": [], "batched_build": [], "loop": []}
    steps = {}
    evs = {}
    for name, graph in (("batched_graph", True), ("batched_eager", False)):
        t0 = time.time()
        evs[name] = Evaluator(PolicySet(pols, "fp32", device), [n] * K, per_policy_env_kwargs=per, seed=0, graph=graph)
        evs[name].evaluate()  # warm-up (and the capture)
        torch.cuda.synchronize()
        res["batched_build"].append(time.time() - t0)
    loop_eval(pols[:1], n, 0, device)  # warm-up
    for _ in range(repeats):
        for name in ("batched_graph", "batched_eager"):
            torch.cuda.synchronize()
            t0 = time.time()
            r = evs[name].evaluate()
            torch.cuda.synchronize()
            res[name].append(time.time() - t0)
            steps[name] = sum(x["env_steps"] for x in r)
        torch.cuda.synchronize()
        t0 = time.time()
        steps["loop"] = loop_eval(pols, n, 0, device)
        torch.cuda.synchronize()
        res["loop"].append(time.time() - t0)
    for ev in evs.values():
        ev.close()
    out = {k: stats(v) for k, v in res.items()}
    out["env_steps"] = steps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=15)
    ap.add_argument("--envs", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--eval-repeats", type=int, default=2)
    ap.add_argument("--arms", default="ab")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = nat.require_gpu("cuda:0")
    res = dict(policies=a.policies, envs=a.envs)
    if "a" in a.arms:
        for prec in ("bf16", "fp32"):
            r = res[f"select_{prec}_ms"] = arm_a(prec, a.policies, a.envs, a.repeats, a.iters, dev)
            for k, v in r.items():
                print(f"(a) {prec:5s} {k:7s} ms per {a.policies} x {a.envs} rows: min {v['min']:.4f} median {v['median']:.4f} "
                      f"max {v['max']:.4f}  ({v['n']} x {a.iters})", flush=True)
    if "b" in a.arms:
        r = res["evaluation_s"] = arm_b(a.policies, a.envs, a.eval_repeats, dev)
        for k, v in r.items():
            if k != "env_steps":
                print(f"(b) {k:14s} s: min {v['min']:.3f} median {v['median']:.3f} max {v['max']:.3f}  ({v['n']})",
                      flush=True)
        print("(b) env steps:", r["env_steps"], flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
