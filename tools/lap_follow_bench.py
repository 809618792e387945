"""What live views (LAP.view(..., live=True), lap_views_follow) cost an insert,
against rebuilding the views, and what they cost a Collector.

    python tools/lap_follow_bench.py                  # both parts
    python tools/lap_follow_bench.py --skip-collector # the inserts only

1. us per add_batch(source=...) of --rows rows (12,000) spread evenly over 8
   full strata of --capacity slots with 0, 1 and 15 live views attached (view p
   keeps source p of 15), by device events around one call, the device idle
   before each, median of --repeats after a warm-up; and, in the same process
   on the same buffer, the time of 15 rebuild() calls -- what keeping 15
   snapshot views current after one insert costs today -- by device events and
   by the host clock (rebuild() reads the source counts on the host).
2. Seconds per --steps (1,000) steps of a Collector of 15 stand-in policies x
   800 envs (bf16, graph=True unless --eager, tag_sources=True) on a replay
   with 0 and with 15 live views, alternating, --collect-repeats times each.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "a-deep-reinforcement-learning-enabled-soft-exoskeleton-for-parkinson-s-patients_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

K = 15


def stats(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 2), median=round(xs[len(xs) // 2], 2), max=round(xs[-1], 2), n=len(xs))


def timed(fn, repeats, warm=3):
    """us of `repeats` single calls by device events (the device idle before each)"""
    for _ in range(warm):
        fn()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return stats(us)


def inserts(a, dev):
    from exo_amd.replay import LAP
    E, C, n = 8, a.capacity, a.rows
    base = LAP(80, 7, dev, E, max_size=C, batch_size=128)
    g = torch.Generator(device=dev).manual_seed(0)
    strata = torch.arange(n, device=dev, dtype=torch.int32) % E
    st, ac = torch.randn((n, 80), device=dev, generator=g), torch.rand((n, 7), device=dev, generator=g)
    rw = torch.randn((n,), device=dev, generator=g)
    done = torch.zeros(n, dtype=torch.uint8, device=dev)
    src = torch.randint(0, K, (n,), device=dev, generator=g, dtype=torch.int32)

    def add():
        base.add_batch(st, ac, st, rw, done, strata, source=src)
    for _ in range((E * C + n - 1) // n):
        add()
    torch.cuda.synchronize()
    assert base.size_s.tolist() == [C] * E
    out = dict(strata=E, capacity=C, cap=base._cap, rows=n, sources=K)
    out["add_batch_us_0_views"] = timed(add, a.repeats)
    views = [base.view([0], live=True)]
    out["add_batch_us_1_view"] = timed(add, a.repeats)
    views += [base.view([p], live=True) for p in range(1, K)]
    out["add_batch_us_15_views"] = timed(add, a.repeats)
    # the same views kept current the old way: every one rebuilt after the insert
    host = []
    torch.cuda.synchronize()
    followed = [(v._tree.clone(), v.kept.clone()) for v in views[:2]]

    def rebuild_all():
        t0 = time.perf_counter()
        for v in views:
            v.rebuild()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    out["rebuild_15_views_us_events"] = timed(rebuild_all, a.repeats)
    out["rebuild_15_views_us_host"] = stats(host[3:])
    # the followed trees are the rebuilt ones (no priority was updated)
    assert all(torch.equal(v._tree, t) and torch.equal(v.kept, k) for v, (t, k) in zip(views, followed))
    for v in views:
        v.detach()
    out["add_batch_us_0_views_after"] = timed(add, a.repeats)
    return out


def collector(a, dev):
    from eval_bench import CONFIGS, stand_ins
    from exo_amd import Collector
    from exo_amd.fused import PolicySet
    from exo_amd.replay import LAP
    pols = stand_ins(K, dev)
    arms = {}
    for name, nv in (("0_views", 0), ("15_views", K)):
        rb = LAP(80, 7, dev, 8, max_size=a.collect_capacity, batch_size=128)
        col = Collector(PolicySet(pols, "bf16", dev, None), [a.envs] * K, rb, sigma=0.1,
                        per_policy_env_kwargs=[dict(tremor_sequence=CONFIGS[k]) for k in range(K)],
                        graph=not a.eager, tag_sources=True)
        views = [rb.view([p], live=True) for p in range(nv)]
        col.collect(a.steps)  # warm-up and the captures
        arms[name] = (col, rb, views)
    t = {k: [] for k in arms}
    for _ in range(a.collect_repeats):
        for name, (col, _, _) in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            col.collect(a.steps)
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    out = dict(policies=K, envs_per_policy=a.envs, steps=a.steps, graph=not a.eager, capacity=a.collect_capacity)
    for name, (col, rb, views) in arms.items():
        xs = sorted(t[name])
        out[f"collect_s_{name}"] = dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4),
                                        n=len(xs))
        if views:  # each policy's view keeps exactly its rows
            counts = rb.source_counts(K)[:, :K].cpu()
            assert all(v.kept.cpu().tolist() == counts[:, p].tolist() for p, v in enumerate(views))
        col.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=250_000)
    ap.add_argument("--rows", type=int, default=12_000)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--envs", type=int, default=800, help="envs per policy of the collector part")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--collect-repeats", type=int, default=5)
    ap.add_argument("--collect-capacity", type=int, default=25_000)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--skip-collector", action="store_true")
    a = ap.parse_args()
    from exo_amd import _native as nat
    dev = nat.require_gpu("cuda:0")
    res = dict(metric="lap_views_follow", inserts=inserts(a, dev))
    if not a.skip_collector:
        res["collector"] = collector(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
