"""Deterministic evaluation of many policies as one env batch.

Evaluator owns one VecExoskeletonEnv whose envs are split into contiguous
segments, one per policy of a fused.PolicySet, and runs every env for one
episode: each step is one td7f_select_multi launch (every policy acts on its
own rows), env.step, env.eval_metrics and the return / step-count sums, all on
one stream -- what tools/eval_policies.py does per configuration with torch
modules (Simulation/Evaluate_control_performance.py), for all configurations
at once.  No exploration, no agent state touched.
"""
import numpy as np
import torch

from . import graphs
from .vec_env import VecExoskeletonEnv


def segment_layout(K, envs_per_policy, env_kwargs=None, per_policy_env_kwargs=None, owner="Evaluator"):
    """One env batch for K policies (Evaluator, Collector): policy p's envs are
    the contiguous rows [seg[p], seg[p+1]), env i of a segment follows motion
    i % 8, env_kwargs go to every env and per_policy_env_kwargs[p] (a dict) to
    policy p's envs, concatenated per segment.  envs_per_policy: one count or
    K.  Returns (seg: K + 1 ints, motions: int64 [n], the env keyword
    arguments).  Host only."""
    if isinstance(envs_per_policy, (int, np.integer)):
        envs_per_policy = [int(envs_per_policy)] * K
    counts = [int(c) for c in envs_per_policy]
    if len(counts) != K or min(counts) < 0 or sum(counts) <= 0:
        raise ValueError(f"{owner}: envs_per_policy must hold {K} non-negative counts, not all zero")
    seg = [0] + [int(v) for v in np.cumsum(counts)]
    kw = dict(env_kwargs or {})
    if per_policy_env_kwargs is not None:
        if len(per_policy_env_kwargs) != K:
            raise ValueError(f"{owner}: per_policy_env_kwargs must hold {K} dicts")
        names = set().union(*[set(d) for d in per_policy_env_kwargs])
        for name in names:
            if any(name not in d for d in per_policy_env_kwargs):
                raise ValueError(f"{owner}: per_policy_env_kwargs: {name!r} is not given for every policy")
            vals = [np.asarray(d[name], dtype=np.float64) for d in per_policy_env_kwargs]
            kw[name] = np.concatenate([np.broadcast_to(v, (c,) + v.shape) for v, c in zip(vals, counts)], axis=0)
    motions = np.concatenate([np.arange(c) % 8 for c in counts]).astype(np.int64)
    return seg, motions, kw


class Evaluator:
    """Evaluator(policy_set, envs_per_policy, ...): policy p's envs are the
    contiguous rows [seg[p], seg[p+1]) of one VecExoskeletonEnv; env i of a
    segment follows motion i % 8.  env_kwargs go to every env,
    per_policy_env_kwargs[p] (a dict) to policy p's envs -- e.g. each shipped
    configuration's tremor_sequence.

    graph=True replays the step from one graph captured on a single stream
    (graphs.new_graph / graphs.capture; no forks, no side streams); release()
    destroys it through graphs.release_graphs.  Off by default: at 15 x 800
    envs the replayed and the eager step take the same time
    (profiles/eval_multi), the device work bounds the loop."""

    def __init__(self, policy_set, envs_per_policy, env_kwargs=None, per_policy_env_kwargs=None, seed=0,
                 physics="ideal", max_action=1.0, graph=False):
        K = len(policy_set)
        self.seg, motions, kw = segment_layout(K, envs_per_policy, env_kwargs, per_policy_env_kwargs, "Evaluator")
        self.policy_set = policy_set
        self.n = self.seg[-1]
        self.seed = int(seed)
        self.max_action = float(max_action)
        self.device = policy_set.dev
        self.env = VecExoskeletonEnv(self.n, motions=motions, seed=self.seed, device=self.device, physics=physics,
                                     **kw)
        d = self.device
        self._out = self.env.new_outputs(True)
        self._act = torch.zeros((self.n, policy_set.A), dtype=torch.float32, device=d)
        self._active = torch.zeros(self.n, dtype=torch.bool, device=d)
        self._active_f = torch.zeros(self.n, dtype=torch.float32, device=d)
        self.counters = torch.zeros((self.n, 5), dtype=torch.float32, device=d)
        self.returns = torch.zeros(self.n, dtype=torch.float32, device=d)
        self.steps = torch.zeros(self.n, dtype=torch.float32, device=d)
        self.use_graph = bool(graph)
        self._graph = None
        self._evaluated = False
        policy_set.tiles(self.seg)  # the tile table, before any capture

    @classmethod
    def from_agent(cls, agent, n_envs, use_checkpoint=True, **env):
        """One policy (K = 1): the agent's checkpoint policy (use_checkpoint=
        False: its live one) on n_envs envs; env: Evaluator's keyword arguments
        (seed, physics, graph) and env arguments."""
        from .fused import PolicySet
        own = {k: env.pop(k) for k in ("seed", "physics", "graph") if k in env}
        ps = PolicySet.from_agents([agent], use_checkpoint=use_checkpoint)
        return cls(ps, [int(n_envs)], env_kwargs=env, max_action=agent.max_action, **own)

    @property
    def done(self):
        """the envs' done flags after the last evaluate() (bool [n])"""
        return self._out[2].view(torch.bool)

    def _step(self):
        obs, rew, done, info = self._out
        torch.eq(done, 0, out=self._active)
        self._active_f.copy_(self._active)
        self.policy_set.act(obs, self.seg, out=self._act, scale=self.max_action)
        self.env.step(self._act, active=self._active, out=self._out)
        self.env.eval_metrics(info, stepped=self._active, counters=self.counters)
        self.returns.addcmul_(rew, self._active_f)
        self.steps.add_(self._active_f)

    def _capture(self):
        cur = torch.cuda.current_stream(self.device)
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(cur)
        g = graphs.new_graph()
        with torch.cuda.stream(s):
            with graphs.capture(g, stream=s):
                self._step()
        cur.wait_stream(s)
        self._graph = g

    @torch.no_grad()
    def evaluate(self, episodes=None):
        """Every env for one episode, deterministically.  Returns a list with
        one dict per policy: return_mean, return_min, env_steps, the sums of
        VecExoskeletonEnv.EVAL_COUNTER_NAMES and -- with episodes given, the
        policy's envs being 8 x episodes (env e: motion e % 8 of episode
        e // 8) -- the evaluation script's metrics occurrence / total /
        torque_any / torque_all as [mean, std] over the episodes.  Every
        policy's weights are repacked from the modules first (PolicySet.pack),
        so the call sees the modules as they are now, whoever wrote them
        (torch, the HIP optimisers, a replayed graph).  A repeated
        call first puts the env back where its constructor left it
        (VecExoskeletonEnv.restart, ideal physics only), so it sees the same
        episodes."""
        env = self.env
        with torch.cuda.device(self.device):
            if self._evaluated:
                env.restart(self.seed)
            self._evaluated = True
            obs, rew, done, _ = self._out
            env.reset(obs_out=obs)
            rew.zero_()
            done.zero_()
            for t in (self.counters, self.returns, self.steps):
                t.zero_()
            # always: the HIP optimisers and graph replays write the master
            # weights without moving a torch version counter (refresh() sees
            # only torch's writes), and a pack is a few launches
            self.policy_set.pack()
            k0 = 0
            if self.use_graph and self._graph is None:
                self._step()  # once eagerly, then recorded
                self._capture()
                k0 = 1
            for _ in range(k0, env.max_len):
                if self._graph is not None:
                    self._graph.replay()
                else:
                    self._step()
            if not bool(self.done.all()):
                raise RuntimeError("Evaluator: episodes did not finish within max_len steps")
        c = self.counters.double().cpu().numpy()
        ret = self.returns.double().cpu().numpy()
        steps = self.steps.double().cpu().numpy()
        res = []
        for p in range(len(self.policy_set)):
            a, b = self.seg[p], self.seg[p + 1]
            r = dict(policy=p, envs=b - a, env_steps=int(steps[a:b].sum()),
                     return_mean=float(ret[a:b].mean()) if b > a else float("nan"),
                     return_min=float(ret[a:b].min()) if b > a else float("nan"))
            for j, name in enumerate(env.EVAL_COUNTER_NAMES):
                r[name] = float(c[a:b, j].sum())
            if episodes is not None:
                if b - a != 8 * int(episodes):
                    raise ValueError(f"Evaluator.evaluate: policy {p} has {b - a} envs, not 8 x {episodes}")
                r.update(episode_metrics(c[a:b], int(episodes), env.lengths_host[a:a + 8]))
            res.append(r)
        return res

    def release(self):
        """Destroy the step graph (graphs.release_graphs; synchronises)."""
        g, self._graph = self._graph, None
        return graphs.release_graphs(g) if g is not None else 0

    def close(self):
        self.release()
        self.env.close()


def episode_metrics(counters, episodes, lengths8):
    """The EVALUATION METRICS of Simulation/Evaluate_control_performance.py
    :421-426 from the eval_metrics counters [8 x episodes, 5] (env e: motion
    e % 8 of episode e // 8), per episode, as [mean, std] over the episodes --
    the expressions of tools/eval_policies.py."""
    c = np.asarray(counters, dtype=np.float64).reshape(episodes, 8, 5).sum(1)
    denom = float((np.asarray(lengths8) - 3).sum())  # total_steps_for_ep (:95-96)
    occ = c[:, 2] / (c[:, 2] + c[:, 3]) * 100
    tot = c[:, 4] / np.maximum(c[:, 2], 1)
    any_ = c[:, 1] / denom * 100
    all_ = c[:, 0] / denom * 100
    return dict(total=[float(tot.mean()), float(tot.std())], occurrence=[float(occ.mean()), float(occ.std())],
                torque_any=[float(any_.mean()), float(any_.std())], torque_all=[float(all_.mean()), float(all_.std())])
