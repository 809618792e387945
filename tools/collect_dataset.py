"""Collect an offline dataset from several noisy behaviour policies, all acting
in one env batch (exo_amd.Collector: one td7f_select_multi_noise launch per
step, every policy with its own sigma and random stream), into a fresh
Agent(..., offline=True)'s replay, and write it with Agent.save_dataset -- the
file Agent.load_dataset / OfflineTrainer train from.

Policies: --dir, the shipped ones (policies/*.safetensors, tools/eval_policies.py's
loader, each on its own tremor configuration with the evaluation script's env
arguments), or --stand-ins K, the seeded stand-in policies of tools/eval_bench.py.

Prints one JSON line: transitions, episodes and return per policy, and
transitions per second.

--bench times Collector.collect against the per-policy loop it replaces: K
single-policy collectors, each with its own env and its own td7f_select launch
per step, run one after the other over the same policies and env counts.  The
two arms alternate in one process, per precision (bf16, fp32); seconds by a
host clock around a device synchronise.

--noise pink collects with one coloured noise sequence per env and episode
(fused.PinkNoise, exponent --beta) instead of white noise.  --bench --noise pink
times three collectors at one shape, alternating: the pink one, the Gaussian
one, and ComposedPinkCollector, pink noise from the pieces that need the host
every step (read done, hipFFT for the finished envs, gather, given normals).

--tag-sources records which policy produced every row (Collector(tag_sources=True):
the replay's source column, a `source` key in the dataset file), for
LAP.view / LAP.source_counts; with --bench both arms tag their rows (the loop
arm's single-policy collectors as policy 0).

usage: python tools/collect_dataset.py (--dir DIR | --stand-ins K) [--sigma S [S ...]] [--envs-per-policy 64]
                                       [--steps 500] [--precision fp32] [--noise pink [--beta 1.0]] [--tag-sources]
                                       [--out FILE]
       python tools/collect_dataset.py --bench [--stand-ins 15] [--envs-per-policy 800] [--steps 100]
                                       [--repeats 5] [--graph] [--noise pink] [--tag-sources] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "a-deep-reinforcement-learning-enabled-soft-exoskeleton-for-parkinson-s-patients_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from exo_amd import Collector  # noqa: E402
from exo_amd import _native as nat  # noqa: E402
from exo_amd.fused import PolicySet, TD7FNoise  # noqa: E402
from exo_amd.td7 import Agent, Hyperparameters  # noqa: E402


def load_policies(a, device):
    """(module pairs, activations, env_kwargs, per_policy_env_kwargs)"""
    if a.dir:
        from eval_policies import EVAL_ENV, policy
        files = [f for f in sorted(os.listdir(a.dir)) if f.endswith(".safetensors")]
        if not files:
            raise SystemExit(f"no *.safetensors under {a.dir}")
        hp = Hyperparameters(actor_hdim=300)
        seqs = [[int(c) for c in f[:-len(".safetensors")].strip("[]").split(",")] + [0, 0, 0] for f in files]
        return ([policy(os.path.join(a.dir, f), device) for f in files], (hp.enc_activ, hp.actor_activ), EVAL_ENV,
                [dict(tremor_sequence=s) for s in seqs])
    from eval_bench import CONFIGS, stand_ins
    K = a.stand_ins
    return stand_ins(K, device), None, None, [dict(tremor_sequence=CONFIGS[k % 15]) for k in range(K)]


def fresh_agent(per, steps, precision, device):
    """an offline agent whose replay holds per x steps transitions per policy without wrapping"""
    K = len(per)
    rows = max(int(np.bincount(np.concatenate([np.arange(c) % 8 for c in per]), minlength=8).max()) * steps, 64)
    return Agent(80, 7, 1, offline=True, env_num=8, device=device, buffer_size=rows, precision=precision), K


class SingleCollector(Collector):
    """The loop arm's collector: one policy, its own env, and td7f_select (the
    single-policy launch, the library's tile pick) for the actions; everything
    else of the step is Collector's."""

    def _select(self, obs):
        ps, mn = self.policy_set, self.noise
        r = mn.rngs[0]
        nz = TD7FNoise(r.seed, r.tag, 0, r.counter_ptr, r.ticket_ptr, mn.sigmas[0].data_ptr(), mn.sigma_dec[0], mn.clip[0],
                       self.max_action, 0, None, None)
        nat.check(nat.lib().td7f_select(ps.prec, ps.act_codes, ps.enc, ps.actor, nat.ptr(obs), self.n, ctypes.byref(nz),
                                        nat.ptr(self._act), 0, 0, nat.stream_ptr(self.device)), "td7f_select")
        return self._act


def stats(xs):
    xs = sorted(xs)
    return dict(min=xs[0], median=xs[len(xs) // 2], max=xs[-1], n=len(xs))


def bench(a, device):
    pols, activ, env_kw, per_kw = load_policies(a, device)
    K, n = len(pols), a.envs_per_policy
    res = dict(policies=K, envs_per_policy=n, steps=a.steps, graph=bool(a.graph))
    for prec in ("bf16", "fp32"):
        ag, _ = fresh_agent([n] * K, 8, prec, device)  # a ring: the timing does not need every row kept
        rb = ag.replay_buffer
        multi = Collector(PolicySet(pols, prec, device, activ), [n] * K, rb, sigma=a.sigma[0], env_kwargs=env_kw,
                          per_policy_env_kwargs=per_kw, graph=a.graph, tag_sources=a.tag_sources)
        singles = [SingleCollector(PolicySet([pols[k]], prec, device, activ), [n], rb, sigma=a.sigma[0],
                                   env_kwargs=env_kw, per_policy_env_kwargs=[per_kw[k]], graph=a.graph,
                                   tag_sources=a.tag_sources) for k in range(K)]

        def run_multi():
            multi.collect(a.steps)

        def run_loop():
            for c in singles:
                c.collect(a.steps)
        arms = dict(multi=run_multi, loop=run_loop)
        for fn in arms.values():  # warm-up (and the captures)
            fn()
        t = {k: [] for k in arms}
        for _ in range(a.repeats):
            for name, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.time()
                fn()
                torch.cuda.synchronize()
                t[name].append(time.time() - t0)
        r = res[f"collect_{prec}_s"] = {k: stats(v) for k, v in t.items()}
        r["transitions"] = K * n * a.steps
        for k in arms:
            v = r[k]
            print(f"{prec:5s} {k:6s} s per {K} x {n} envs x {a.steps} steps: min {v['min']:.4f} median {v['median']:.4f} "
                  f"max {v['max']:.4f}  ({v['n']})  {r['transitions'] / v['median']:.3g} transitions/s", flush=True)
        for c in [multi] + singles:
            c.close()
        del multi, singles, ag, rb
        torch.cuda.empty_cache()
    return res


class ComposedPinkCollector(Collector):
    """Pink noise per env from the pieces that exist without td7f_pink_advance:
    each step the host reads `done`, the finished envs' sequences are drawn
    anew with pink.powerlaw_psd_gaussian_device (torch.randn + hipFFT, one call
    per motion length among them) and peak-normalised, column t of every env's
    sequence is gathered into z, and PolicySet.act(noise=MultiNoise, z=z) adds
    z * sigma.  The host read rules graph replay out; everything else of the
    step is Collector's."""

    def __init__(self, *args, beta=1.0, **kw):
        kw["graph"] = False
        super().__init__(*args, **kw)
        self.beta = float(beta)
        self._len = np.asarray(self.env.lengths_host)
        A = self.policy_set.A
        self._seq = torch.zeros((self.n, A, int(self._len.max())), dtype=torch.float32, device=self.device)
        self._t = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        self._rows = torch.arange(self.n, device=self.device)
        self._last_done = None
        self._regenerate(np.arange(self.n))

    def _regenerate(self, ids):
        from exo_amd import pink
        A = self.policy_set.A
        for n in np.unique(self._len[ids]):
            rows = ids[self._len[ids] == n]
            x = pink.powerlaw_psd_gaussian_device(self.beta, len(rows) * A, int(n), self.device).view(len(rows), A, int(n))
            x = x / x.abs().amax(dim=(1, 2), keepdim=True)
            self._seq[torch.as_tensor(rows, device=self.device), :, :int(n)] = x

    def _select(self, obs):
        if self._last_done is not None:
            ids = np.flatnonzero(self._last_done.cpu().numpy())  # the host read of every step
            if ids.size:
                self._regenerate(ids)
                self._t[torch.as_tensor(ids, device=self.device)] = 0
        z = self._seq[self._rows, :, self._t].contiguous()
        self._t += 1
        return self.policy_set.act(obs, self.seg, out=self._act, scale=self.max_action, noise=self.noise, z=z)

    def _step(self, c):
        super()._step(c)
        self._last_done = self._outs[c][2]


def bench_pink(a, device):
    """--bench --noise pink: the pink Collector, the Gaussian Collector and the
    composed baseline (ComposedPinkCollector) at one shape, alternating."""
    pols, activ, env_kw, per_kw = load_policies(a, device)
    K, n = len(pols), a.envs_per_policy
    res = dict(policies=K, envs_per_policy=n, steps=a.steps, graph=bool(a.graph), noise="pink", beta=a.beta)
    for prec in ("bf16", "fp32"):
        ag, _ = fresh_agent([n] * K, 8, prec, device)  # a ring: the timing does not need every row kept
        rb = ag.replay_buffer
        kw = dict(sigma=a.sigma[0], env_kwargs=env_kw, per_policy_env_kwargs=per_kw)
        cols = dict(pink=Collector(PolicySet(pols, prec, device, activ), [n] * K, rb, graph=a.graph, noise="pink",
                                   beta=a.beta, **kw),
                    gaussian=Collector(PolicySet(pols, prec, device, activ), [n] * K, rb, graph=a.graph, **kw),
                    composed=ComposedPinkCollector(PolicySet(pols, prec, device, activ), [n] * K, rb, beta=a.beta, **kw))
        for c in cols.values():  # warm-up (and the captures)
            c.collect(a.steps)
        t = {k: [] for k in cols}
        for _ in range(a.repeats):
            for name, c in cols.items():
                torch.cuda.synchronize()
                t0 = time.time()
                c.collect(a.steps)
                torch.cuda.synchronize()
                t[name].append(time.time() - t0)
        r = res[f"collect_{prec}_s"] = {k: stats(v) for k, v in t.items()}
        r["transitions"] = K * n * a.steps
        for k in cols:
            v = r[k]
            print(f"{prec:5s} {k:8s} s per {K} x {n} envs x {a.steps} steps: min {v['min']:.4f} median {v['median']:.4f} "
                  f"max {v['max']:.4f}  ({v['n']})  {r['transitions'] / v['median']:.3g} transitions/s", flush=True)
        for c in cols.values():
            c.close()
        del cols, ag, rb
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    src = ap.add_mutually_exclusive_group()
    src.add_argument("--dir", default=None, help="the shipped policies (*.safetensors)")
    src.add_argument("--stand-ins", type=int, default=None, help="K seeded stand-in policies")
    ap.add_argument("--sigma", type=float, nargs="+", default=[0.1], help="one value, or one per policy")
    ap.add_argument("--sigma-dec", type=float, default=0.0)
    ap.add_argument("--clip", type=float, default=0.0)
    ap.add_argument("--envs-per-policy", type=int, default=None)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--precision", default="fp32", choices=("bf16", "fp16", "fp32"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--graph", action="store_true", help="replay the step from graphs")
    ap.add_argument("--noise", default="gaussian", choices=("gaussian", "pink"),
                    help="white Gaussian noise per policy, or one coloured sequence per env and episode")
    ap.add_argument("--beta", type=float, default=1.0, help="exponent of the coloured noise's power law (1: pink)")
    ap.add_argument("--tag-sources", action="store_true",
                    help="record the behaviour policy of every row (LAP.view / source_counts; a `source` key in --out)")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = nat.require_gpu("cuda:0")
    if a.bench:
        a.stand_ins = a.stand_ins or (None if a.dir else 15)
        a.envs_per_policy = a.envs_per_policy or 800
        a.steps = a.steps or 100
        line = json.dumps(bench_pink(a, dev) if a.noise == "pink" else bench(a, dev))
        print(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return
    if not a.dir and not a.stand_ins:
        ap.error("one of --dir and --stand-ins is needed")
    a.envs_per_policy = a.envs_per_policy or 64
    a.steps = a.steps or 500
    pols, activ, env_kw, per_kw = load_policies(a, dev)
    K = len(pols)
    sigma = a.sigma[0] if len(a.sigma) == 1 else a.sigma
    torch.manual_seed(a.seed)
    ag, _ = fresh_agent([a.envs_per_policy] * K, a.steps, a.precision, dev)
    col = Collector(PolicySet(pols, a.precision, dev, activ), a.envs_per_policy, ag.replay_buffer, sigma=sigma,
                    sigma_dec=a.sigma_dec, clip=a.clip, env_kwargs=env_kw, per_policy_env_kwargs=per_kw, seed=a.seed,
                    graph=a.graph, noise=a.noise, beta=a.beta, tag_sources=a.tag_sources)
    try:
        torch.cuda.synchronize()
        t0 = time.time()
        rep = col.collect(a.steps)
        torch.cuda.synchronize()
        dt = time.time() - t0
    finally:
        col.close()
    n = sum(r["transitions"] for r in rep)
    if a.out:
        ag.save_dataset(a.out)
    print(json.dumps(dict(policies=K, envs_per_policy=a.envs_per_policy, steps=a.steps, precision=a.precision,
                          noise=a.noise, transitions=n, seconds=dt, transitions_per_s=n / dt, out=a.out, per_policy=rep)))


if __name__ == "__main__":
    main()
