"""Datasets from many noisy behaviour policies in one env batch.

Collector owns one VecExoskeletonEnv whose envs are split into contiguous
segments, one per policy of a fused.PolicySet (Evaluator's layout), and fills a
replay.LAP with their transitions: each step is one td7f_select_multi_noise
launch (every policy acts on its own rows with its own sigma, clip, decay and
random stream: TD7_multi_agent.py:192-209 per policy), env.step, the insert,
the per-env return sums and the in-place resets of finished envs -- all on one
stream, with asynchronous episodes as VecTrainer(episodes="async") runs them.
The replay it fills is what Agent(..., offline=True) / OfflineTrainer train
from and Agent.save_dataset writes.
"""
import numpy as np
import torch

from . import graphs
from .evaluate import segment_layout

PHYSICS = ("ideal", "multibody")
NOISES = ("gaussian", "pink")


def check_sigma_schedule(sigma, sigma_dec, steps, counts=None):
    """ValueError if `steps` more launches would take some sigma below 0:
    policy p (with envs: counts[p] > 0) ends at sigma[p] - steps * sigma_dec[p].
    Host only, from the values given (fp64; a relative 1e-9 of slack for the
    products' rounding)."""
    steps = int(steps)
    if steps < 0:
        raise ValueError("Collector: steps must be >= 0")
    for p, (s, d) in enumerate(zip(sigma, sigma_dec)):
        if counts is not None and counts[p] <= 0:
            continue
        if s - steps * d < -1e-9 * max(s, 1e-30):
            raise ValueError(f"Collector: policy {p}: sigma {s:g} - {steps} x sigma_dec {d:g} falls below 0")


def default_strata(motions, num_strata):
    """The replay stratum of every env, motions % num_strata (int32 [n]), as
    VecTrainer stratifies."""
    return (np.asarray(motions, dtype=np.int64) % int(num_strata)).astype(np.int32)


class Collector:
    """Collector(policy_set, envs_per_policy, replay, sigma=..., ...): policy
    p's envs are the contiguous rows [seg[p], seg[p+1]) of one
    VecExoskeletonEnv, env i of a segment on motion i % 8; env_kwargs go to
    every env, per_policy_env_kwargs[p] to policy p's (evaluate.segment_layout).
    sigma, sigma_dec, clip: scalars or one value per policy (fused.MultiNoise,
    which the collector owns: policy p draws from tag MULTI_NOISE_TAG0 + p).
    noise="pink": instead of white noise, one coloured sequence (power-law
    exponent beta) per env and episode, of the env's motion length, scaled by
    its policy's sigma at the episode's start (fused.PinkNoise;
    TD7_multi_agent_Pink_noise.py:203-228); after the statistics of a step one
    td7f_pink_advance launch counts the steps and regenerates the sequences of
    the envs that finished, on the device.

    replay: a replay.LAP of the policies' state / action dimensions, e.g.
    agent.replay_buffer; env i's rows go to stratum strata[i] (int32 [n],
    default motions % replay.num_envs).

    graph=True replays the step from graphs captured on a single stream, one
    per observation-buffer parity (graphs.new_graph / graphs.capture; no forks,
    no side streams); release() destroys them through graphs.release_graphs.

    tag_sources=True: the replay records which policy produced every row
    (replay.enable_sources(); add_batch(source=...) with env i's policy, an
    int32 device tensor built once from seg) -- the same launches per step --
    so replay.view([p]) is policy p's dataset and replay.source_counts(K) its
    size per stratum.  replay.view([p], live=True) follows the collection: the
    insert's extra launch (lap_views_follow) is part of the step, recorded with
    it under graph=True, and collect() records the step graphs again when views
    were attached or detached since (replay.live_generation)."""

    def __init__(self, policy_set, envs_per_policy, replay, sigma=0.1, sigma_dec=0.0, clip=0.0, env_kwargs=None,
                 per_policy_env_kwargs=None, seed=0, physics="ideal", max_action=1.0, strata=None, graph=False,
                 noise="gaussian", beta=1.0, tag_sources=False):
        from .fused import MultiNoise, PinkNoise, per_policy
        from .vec_env import VecExoskeletonEnv
        K = len(policy_set)
        if physics not in PHYSICS:
            raise ValueError(f"Collector: physics must be one of {PHYSICS}, not {physics!r}")
        if noise not in NOISES:
            raise ValueError(f"Collector: noise must be one of {NOISES}, not {noise!r}")
        sig = per_policy(sigma, K, "sigma", "Collector")
        dec = per_policy(sigma_dec, K, "sigma_dec", "Collector")
        per_policy(clip, K, "clip", "Collector")
        self.seg, motions, kw = segment_layout(K, envs_per_policy, env_kwargs, per_policy_env_kwargs, "Collector")
        self.counts = [b - a for a, b in zip(self.seg[:-1], self.seg[1:])]
        if (replay.state_dim, replay.action_dim) != (policy_set.S, policy_set.A):
            raise ValueError(f"Collector: the replay holds ({replay.state_dim}, {replay.action_dim})-dimensional "
                             f"states / actions, the policies ({policy_set.S}, {policy_set.A})")
        self.n = self.seg[-1]
        if strata is None:
            strata_h = default_strata(motions, replay.num_envs)
        else:
            strata_h = np.asarray(strata.cpu() if torch.is_tensor(strata) else strata).astype(np.int64).reshape(-1)
            if strata_h.size != self.n or strata_h.min() < 0 or strata_h.max() >= replay.num_envs:
                raise ValueError(f"Collector: strata must hold {self.n} values in 0..{replay.num_envs - 1}")
            strata_h = strata_h.astype(np.int32)
        if np.bincount(strata_h, minlength=replay.num_envs).max() > replay.max_size:
            raise ValueError("Collector: one step's rows of a stratum exceed the replay's max_size")
        self.policy_set, self.replay = policy_set, replay
        self.seed = int(seed)
        self.max_action = float(max_action)
        self.device = d = policy_set.dev
        self._sigma_host, self._dec_host = sig, dec  # the schedule as set here (check_sigma_schedule)
        self.env = VecExoskeletonEnv(self.n, motions=motions, seed=self.seed, device=d, physics=physics, **kw)
        self.noise_kind = noise
        if noise == "pink":
            # one sequence per env, of its motion's length, regenerated on the device when its episode ends
            self.noise = PinkNoise(policy_set, self.seg, self.env.lengths_host, sig, dec, clip, beta=beta)
        else:
            self.noise = MultiNoise(policy_set, sig, dec, clip)
        self.strata = torch.as_tensor(strata_h, device=d)
        self.sources = None
        if tag_sources:
            replay.enable_sources()
            self.sources = torch.as_tensor(np.repeat(np.arange(K, dtype=np.int32), self.counts), device=d)
        # two observation buffers used in alternation (VecTrainer): step c reads
        # obs[c], the env writes the next observation into obs[1 - c]
        o0 = self.env.reset()
        self._obs = [o0, torch.empty_like(o0)]
        outs = [self.env.new_outputs(False), self.env.new_outputs(False)]
        self._outs = [(self._obs[1], *outs[0][1:]), (self._obs[0], *outs[1][1:])]
        self._cur = 0
        self._act = torch.zeros((self.n, policy_set.A), dtype=torch.float32, device=d)
        self.active = torch.ones(self.n, dtype=torch.bool, device=d)
        self.active_count = torch.full((1,), self.n, dtype=torch.int32, device=d)
        self._steps_total = torch.zeros((1,), dtype=torch.int64, device=d)
        # per-env accumulators, elementwise (no atomics): the running episode's
        # return in fp32 in step order (Evaluator.returns' accumulation) and in
        # fp64; over finished episodes their count, fp64 return sum and minimum;
        # the first finished episode's fp32 return (NaN until then)
        f64 = dict(dtype=torch.float64, device=d)
        self._ret32 = torch.zeros(self.n, dtype=torch.float32, device=d)
        self._ret64 = torch.zeros(self.n, **f64)
        self.episodes = torch.zeros(self.n, **f64)
        self.return_sum = torch.zeros(self.n, **f64)
        self.return_min = torch.full((self.n,), float("inf"), **f64)
        self.first_return = torch.full((self.n,), float("nan"), dtype=torch.float32, device=d)
        self._first_open = torch.ones(self.n, dtype=torch.bool, device=d)
        self._d64 = torch.zeros(self.n, **f64)
        self._t64 = torch.zeros(self.n, **f64)
        self._inf64 = torch.full((self.n,), float("inf"), **f64)
        self._tb = torch.zeros(self.n, dtype=torch.bool, device=d)
        self.steps_run = 0
        self.use_graph = bool(graph)
        self._graphs = {}
        self._live_gen = replay.live_generation
        policy_set.tiles(self.seg)  # the tile table and the device seg, before any capture

    @classmethod
    def from_agents(cls, agents, replay, use_checkpoint=True, envs_per_policy=8, **kw):
        """The agents' checkpoint policies (use_checkpoint=False: their live
        ones) as the behaviour policies; kw: Collector's other arguments
        (max_action defaults to the agents')."""
        from .fused import PolicySet
        agents = list(agents)
        ps = PolicySet.from_agents(agents, use_checkpoint=use_checkpoint)
        kw.setdefault("max_action", agents[0].max_action)
        return cls(ps, envs_per_policy, replay, **kw)

    @property
    def obs(self):
        """The current observation buffer."""
        return self._obs[self._cur]

    def _select(self, obs):
        """every policy's noisy actions for its rows: one launch"""
        return self.policy_set.act(obs, self.seg, out=self._act, scale=self.max_action, noise=self.noise)

    def _step(self, c):
        obs = self._obs[c]
        out = self._outs[c]
        act = self._select(obs)
        nobs, rew, done, _ = self.env.step(act, active=self.active, out=out, with_info=False)
        # before the in-place resets: next_state of a done row is the terminal observation
        self.replay.add_batch(obs, act, nobs, rew, done, self.strata, self.active, source=self.sources)
        self._ret32.add_(rew)
        self._ret64.add_(rew)
        self._d64.copy_(done)
        self.episodes.add_(self._d64)
        self.return_sum.addcmul_(self._ret64, self._d64)
        torch.where(done, self._ret64, self._inf64, out=self._t64)
        torch.minimum(self.return_min, self._t64, out=self.return_min)
        torch.logical_and(done, self._first_open, out=self._tb)
        torch.where(self._tb, self._ret32, self.first_return, out=self.first_return)
        self._first_open.logical_xor_(self._tb)
        self._ret32.masked_fill_(done, 0.0)
        self._ret64.masked_fill_(done, 0.0)
        if self.noise_kind == "pink":
            self.noise.advance(self.active, done)
        self.env.episode_advance(self.active, self.active_count, out[0], self._steps_total)

    def _capture(self, c):
        cur = torch.cuda.current_stream(self.device)
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(cur)
        g = graphs.new_graph()
        with torch.cuda.stream(s):
            with graphs.capture(g, stream=s):
                self._step(c)
        cur.wait_stream(s)
        self._graphs[c] = g
        self._live_gen = self.replay.live_generation  # the insert recorded follows this many live views

    def _stepped(self):
        """host bookkeeping of one step: the other buffer, the sigma schedule as set here"""
        self._cur ^= 1
        self.steps_run += 1
        self._sigma_host = [s - d if c > 0 else s for s, d, c in zip(self._sigma_host, self._dec_host, self.counts)]

    @torch.no_grad()
    def step(self):
        """One vectorised step of every env (eager)."""
        with torch.cuda.device(self.device):
            self._step(self._cur)
        self._stepped()

    @torch.no_grad()
    def collect(self, steps):
        """`steps` steps of every env into the replay.  Every policy's weights
        are repacked from the modules first (PolicySet.pack: the HIP optimisers
        and graph replays write the master weights without moving a torch
        version counter).  Returns one dict per policy, over everything this
        collector has run: transitions, episodes finished, return_mean /
        return_min over the finished episodes (NaN if none) and its sigma now.
        One host read, at the end."""
        steps = int(steps)
        check_sigma_schedule(self._sigma_host, self._dec_host, steps, self.counts)
        with torch.cuda.device(self.device):
            self.policy_set.pack()
            k = 0
            if self._graphs and self._live_gen != self.replay.live_generation:
                # live views were attached to or detached from the replay since the
                # capture: the recorded insert follows the old set, record again
                self.release()
            if self.use_graph and len(self._graphs) < 2 and steps >= 2:
                # each parity once eagerly (its buffers exist then), then recorded
                self.step()
                self.step()
                k = 2
                for c in (0, 1):
                    if c not in self._graphs:
                        self._capture(c)
            while k < steps:
                g = self._graphs.get(self._cur) if len(self._graphs) == 2 else None
                if g is None:
                    self.step()
                else:
                    g.replay()
                    self.replay.note_insert()  # the recorded add_batch ran: live views' pending draws are stale
                    self._stepped()
                k += 1
        return self.report()

    def report(self):
        """The per-policy dicts of collect() (one host read)."""
        K = len(self.policy_set)
        host = torch.cat([self.episodes, self.return_sum, self.return_min, self.noise.sigma.double()]).cpu().numpy()
        n = self.n
        eps, rsum, rmin, sig = host[:n], host[n:2 * n], host[2 * n:3 * n], host[3 * n:]
        res = []
        for p in range(K):
            a, b = self.seg[p], self.seg[p + 1]
            e = int(eps[a:b].sum())
            res.append(dict(policy=p, envs=b - a, transitions=(b - a) * self.steps_run, episodes=e,
                            return_mean=float(rsum[a:b].sum() / e) if e else float("nan"),
                            return_min=float(rmin[a:b].min()) if e else float("nan"), sigma=float(sig[p])))
        return res

    def release(self):
        """Destroy the step graphs (graphs.release_graphs; synchronises)."""
        gs, self._graphs = list(self._graphs.values()), {}
        return graphs.release_graphs(*gs) if gs else 0

    def close(self):
        self.release()
        self.env.close()
