"""Contour bridges on one MI355X: how cvs_chain_bridges is timed, and against what.

Inputs, all device arrays: the chains of the thinned contours() edges of a 4096^2 noise frame and the refined positions of chain_refine on
the un-thinned edges map.  The yardstick is cvs_chain_joins on the same arrays in the same process: both calls compute the same arm per
chain end and group ends in a hash table of the same size; the bridges look nine cells up per end instead of one node, compare an end
with up to 32 others per cell, and -- with outputs -- copy the point list and the chain table and append the bridges.  Neither call
synchronises, so each is timed by DEVICE EVENTS around calls repeated over windows of >= 1 s after a warm-up call, the calls alternating
within a round, 3 rounds, medians, all in ONE process.  Nothing is fixed in advance: the probe records what it finds.

  python tools/bridges_probe.py [--window 1.0] [--rounds 3] [--size 4096] [--radius 8] [--max-gap 8] [--min-cos 0.8]
                                [--out profiles/bridges_probe.json]

The row holds ms per call for the bridges with the table only and with outputs and for the joins, the two ratios, ends per ns, and what
the table says (candidates, mutual pairs, junction, short and crowded ends, bridge points)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


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
    xy, _ = f.chain_refine(points, edges)
    n, m = int(points.shape[0]), int(chains.shape[0])
    kw = dict(radius=args.radius, min_arm=min(3, args.radius), max_gap=args.max_gap, min_cos=args.min_cos)
    rec = f.chain_bridges(points, chains, xy=xy, emit=False, **kw)[0]           # the sizing call: the table tells the totals
    lo = (rec["bridge"] >= 0) & (np.arange(len(rec)) < rec["partner"])
    n_bridges, bridge_points = int(lo.sum()), int((rec["steps"][lo] + 1).sum())
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=DEV)
    table_only = (new((2 * m, 32), torch.uint8), new((3,), torch.int32))
    full = (new((2 * m, 32), torch.uint8), new((n + bridge_points, 2), torch.int32), new((m + n_bridges, 4), torch.int32),
            new((n + bridge_points, 2), torch.float32), new((3,), torch.int32))
    join_tab = new((2 * m, 32), torch.uint8)
    import ctypes as C
    from cvsteer_amd import _lib as L
    cfg = L.BridgeCfg(kw["radius"], kw["min_arm"], kw["max_gap"], kw["min_cos"])
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def bridges_table():                                                        # the raw call: the Python method has no table-only out=
        rc = L.lib().cvs_chain_bridges(f._h, ptr(points), n, ptr(chains), m, ptr(xy), C.byref(cfg), ptr(table_only[0]), None, 0, None, 0, None,
                                       ptr(table_only[1]), L.MEM_DEVICE)
        assert rc == 0, rc

    bridges_emit = lambda: f.chain_bridges(points, chains, xy=xy, out=full, **kw)
    joins = lambda: f.chain_joins(points, chains, xy=xy, radius=args.radius, out=join_tab)
    t_tab, t_emit, t_join = [], [], []
    for _ in range(args.rounds):                                                # the calls alternate: what drifts, drifts for all
        t_tab.append(window(torch, bridges_table, args.window))
        t_emit.append(window(torch, bridges_emit, args.window))
        t_join.append(window(torch, joins, args.window))
    t_tab, t_emit, t_join = (statistics.median(t) for t in (t_tab, t_emit, t_join))
    first = [t.cpu().numpy().copy() for t in full]
    bridges_emit()
    torch.cuda.synchronize()
    flags = rec["flags"]
    count = lambda bit: int(((flags & bit) != 0).sum())
    return {"input": "noise %dx%d" % (args.size, args.size), "points": n, "chains": m, **kw,
            "ends": int(((flags & cv.BRIDGE_NONE) == 0).sum()), "junction_ends": count(cv.BRIDGE_JUNCTION), "short_ends": count(cv.BRIDGE_SHORT),
            "crowded_ends": count(cv.BRIDGE_CROWDED), "ends_with_partner": int((rec["partner"] >= 0).sum()), "bridges": n_bridges,
            "bridge_points": bridge_points, "counts": full[4].tolist(), "same_bytes_twice": all(bool((a == t.cpu().numpy()).all()) for a, t in zip(first, full)),
            "scratch_bytes_per_chain": L.BRIDGE_SCRATCH_PER_CHAIN,
            "bridges_table_ms": t_tab, "bridges_emit_ms": t_emit, "chain_joins_ms": t_join,
            "table_over_joins": t_tab / t_join, "emit_over_joins": t_emit / t_join, "table_ends_per_ns": 2 * m / (t_tab * 1e6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--max-gap", type=int, default=8)
    ap.add_argument("--min-cos", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bridges_probe.json"))
    args = ap.parse_args()
    row = measure(args)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump({"method": "device events around calls repeated over >= %.1f s windows after a warm-up call, the calls alternating in one "
                             "process, %d rounds, medians" % (args.window, args.rounds), "rows": [row]}, fp, indent=1)


if __name__ == "__main__":
    main()
