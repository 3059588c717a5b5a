"""Contour joins on one MI355X: how cvs_chain_joins is timed, and against what.

Inputs, all device arrays: the chains of the thinned contours() edges of a 4096^2 noise frame and the refined positions of chain_refine on
the un-thinned edges map.  The yardstick is cvs_chain_measures on the same point list and chain table with the same xy: it touches every
point, the joins touch the chain table and at most `radius` points behind each chain END -- but they also clear and fill a hash table of
16 bytes per slot, 4 to 8 slots per chain, in handle scratch.  Neither call synchronises, so each is timed by DEVICE EVENTS around calls
repeated over windows of >= 1 s after a warm-up call, the calls alternating within a round, 3 rounds, medians, all in ONE process.  Nothing
is fixed in advance: the probe records what it finds.

  python tools/joins_probe.py [--window 1.0] [--rounds 3] [--size 4096] [--radius 8] [--out profiles/joins_probe.json]

The row holds ms per call for the joins and for the measures, their ratio, ends per ns, what the table says (nodes by degree, mutual
joins, short ends) and the bytes the call must move at least -- a floor from shapes, not a kernel's share of peak: per chain 16 bytes of
table entry read and 64 of records written, per end 56 bytes of scratch written by the first launch and read by the third, per slot 16
bytes cleared -- over the time as a fraction of 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
PEAK = 8e12   # bytes per second


def window(torch, fn, seconds):
    """fn repeated until the device events around the calls are >= `seconds` apart -> ms per call"""
    fn()
    torch.cuda.synchronize()
    total, n = 0.0, 0
    while total < 1e3 * seconds:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(64):
            fn()
        t1.record()
        t1.synchronize()
        total += t0.elapsed_time(t1)
        n += 64
    return total / n


def measure(args):
    import numpy as np
    import torch
    import cvsteer_amd as cv
    assert torch.cuda.is_available(), "the probe needs a GPU: there is nothing to time without one"
    torch.manual_seed(1)
    img = torch.rand((args.size, args.size), device=DEV) * 255
    f = cv.SteerableFiltersG2(img)
    edges = f.pipeline(img)[5]
    hi = float(f.nonmax(edges).max())
    mask = f.contours(img, 0.05 * hi, 0.2 * hi)[0]
    points, chains = f.contour_chains(mask)
    xy, strength = f.chain_refine(points, edges)
    n, m = int(points.shape[0]), int(chains.shape[0])
    join_tab = torch.empty((2 * m, 32), dtype=torch.uint8, device=DEV)
    mea_tab = torch.empty((m, 40), dtype=torch.uint8, device=DEV)
    joins = lambda: f.chain_joins(points, chains, xy=xy, radius=args.radius, out=join_tab)
    measures = lambda: f.chain_measures(points, chains, xy=xy, out=mea_tab)
    t_join, t_mea = [], []
    for _ in range(args.rounds):                                                # the calls alternate: what drifts, drifts for both
        t_join.append(window(torch, joins, args.window))
        t_mea.append(window(torch, measures, args.window))
    t_join, t_mea = statistics.median(t_join), statistics.median(t_mea)
    first = join_tab.cpu().numpy().copy()
    joins()
    torch.cuda.synchronize()
    tab = join_tab.cpu().numpy().view(cv.SteerableFiltersG2.JOIN_DTYPE).reshape(-1)
    rep = tab["degree"][tab["node"] == np.arange(len(tab))]                    # one entry per node
    slots = 8
    while slots < 4 * m:
        slots *= 2
    floor = 80.0 * m + 2 * 56.0 * 2 * m + 16.0 * slots
    return {"input": "noise %dx%d" % (args.size, args.size), "radius": args.radius, "points": n, "chains": m, "ends": int((tab["node"] >= 0).sum()),
            "nodes": int(len(rep)), "nodes_by_degree": {str(d): int(c) for d, c in enumerate(np.bincount(rep)) if c},
            "mutual_joins": int(((tab["flags"] & cv.JOIN_MUTUAL) != 0).sum() // 2), "short_ends": int(((tab["flags"] & cv.JOIN_SHORT) != 0).sum()),
            "degenerate_ends": int(((tab["flags"] & cv.JOIN_DEGENERATE) != 0).sum()), "same_bytes_twice": bool((first == join_tab.cpu().numpy()).all()),
            "slots": slots, "scratch_bytes": 112 * m + 16 * slots,
            "chain_joins_ms": t_join, "chain_measures_ms": t_mea, "joins_over_measures": t_join / t_mea,
            "joins_ends_per_ns": 2 * m / (t_join * 1e6), "joins_floor_bytes": floor, "joins_floor_frac_of_peak": floor / (t_join * 1e-3) / PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joins_probe.json"))
    args = ap.parse_args()
    row = measure(args)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump({"method": "device events around calls repeated over >= %.1f s windows after a warm-up call, the calls alternating in one "
                             "process, %d rounds, medians" % (args.window, args.rounds), "rows": [row]}, fp, indent=1)


if __name__ == "__main__":
    main()
