"""us per LAP.view build (lap_view_build) and per LAP.source_counts
(lap_source_counts), by device events, median of --repeats launches after a
warm-up, with the bytes each must move and the HBM bandwidth that implies.

    python tools/lap_view_bench.py                       # 8 x 250,000 and 8 x 1,500,000 slots, full, 15 sources

The kernels read the source column, the ring sizes and (inherit) the base's
leaves and write the view's trees; they never touch the rows, so the buffer is
built with 4 / 1-dimensional rows.  Bytes of a build over full strata: 4 per
slot read (the source), with inherit 4 per leaf of the cap-leaf tree as well
(the base's leaves), and 8 per leaf written (the leaf, and the internal nodes,
cap - 1 of them, once each); the second pass and the keep table are below
0.1 % of that.  source_counts reads 4 bytes per slot.
The fraction of HBM bandwidth is against the 8.0 TB/s peak; a tree that fits
the 256 MiB Infinity Cache (the smaller shape: 2 x 16.8 MB of trees, 8 MB of
sources) is not an HBM measurement and is marked so.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "a-deep-reinforcement-learning-enabled-soft-exoskeleton-for-parkinson-s-patients_amd"))

import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s


def timed(fn, repeats):
    """median us of `repeats` single launches (the device idle before each)"""
    for _ in range(3):
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
    us.sort()
    return dict(min=round(us[0], 2), median=round(us[len(us) // 2], 2), max=round(us[-1], 2), n=len(us))


def shape(E, C, K, repeats, dev):
    from exo_amd import _native as nat
    from exo_amd.replay import LAP
    base = LAP(4, 1, dev, E, max_size=C, batch_size=128)
    g = torch.Generator(device=dev).manual_seed(0)
    chunk = 65536
    strata = (torch.arange(chunk, device=dev, dtype=torch.int32) % E)
    z4, z1 = torch.zeros((chunk, 4), device=dev), torch.zeros((chunk, 1), device=dev)
    done = torch.zeros(chunk, dtype=torch.uint8, device=dev)
    for _ in range((E * C + chunk - 1) // chunk):
        src = torch.randint(0, K, (chunk,), device=dev, generator=g, dtype=torch.int32)
        base.add_batch(z4, z1, z4, z1[:, 0], done, strata, source=src)
    torch.cuda.synchronize()
    assert base.size_s.tolist() == [C] * E
    cap = base._cap
    out = dict(strata=E, capacity=C, cap=cap, sources=K, tree_mb=round(E * 2 * cap * 4 / 1e6, 1))
    v = base.view([0])
    vi = base.view([0], inherit=True)

    def build(view):
        nat.check(nat.lib().lap_view_build(ctypes.byref(view._desc), ctypes.byref(base._desc), ctypes.byref(base._store),
                                           nat.ptr(base.source), nat.ptr(view._keep), view._keep.numel(),
                                           int(view.inherit), base._stream()), "lap_view_build")
    slots = E * C
    cases = dict(view_build=(lambda: build(v), slots * 4 + E * cap * 8),
                 view_build_inherit=(lambda: build(vi), slots * 4 + E * cap * 12),
                 source_counts=(lambda: base.source_counts(K), slots * 4))
    for name, (fn, nbytes) in cases.items():
        t = timed(fn, repeats)
        rate = nbytes / (t["median"] * 1e-6)
        out[name] = dict(us=t, bytes=nbytes, gb_per_s=round(rate / 1e9, 1), hbm_peak_fraction=round(rate / HBM_PEAK, 3))
    out["fits_infinity_cache"] = bool(E * 2 * cap * 4 * 2 + slots * 4 < 256 * 2 ** 20)
    kept = int(base.source_counts(K)[:, 0].sum())
    assert float(v.totals.sum()) == kept  # integer leaves: exact
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strata", type=int, default=8)
    ap.add_argument("--capacity", type=int, nargs="+", default=[250_000, 1_500_000])
    ap.add_argument("--sources", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    from exo_amd import _native as nat
    dev = nat.require_gpu("cuda:0")
    print(json.dumps(dict(metric="lap_view_build_us", shapes=[shape(a.strata, c, a.sources, a.repeats, dev)
                                                             for c in a.capacity])))


if __name__ == "__main__":
    main()
