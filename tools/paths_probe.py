"""Contour paths on one MI355X: how cvs_chain_paths is timed, and against what.

Inputs, all device arrays: the chains of the thinned contours() edges of a 4096^2 noise frame, the refined positions of chain_refine on
the un-thinned edges map and the join table of cvs_chain_joins on them (the input of tools/joins_probe.py and tools/turns_probe.py).  The
yardsticks are cvs_chain_joins and cvs_chain_measures on the same arrays.  None of the three synchronises, so each is timed by DEVICE
EVENTS around calls repeated over windows of >= 1 s after a warm-up call, the calls alternating within a round, 3 rounds, medians, all in
ONE process.  Nothing is fixed in advance: the probe records what it finds.

  python tools/paths_probe.py [--window 1.0] [--rounds 3] [--size 4096] [--radius 8] [--out profiles/paths_probe.json]

The row holds ms per call for the three calls and the two ratios, the launch count and the scratch of the path call, what the result says
(paths, cycles, members of the longest path, points saved) and the bytes the call must move at least -- a floor from shapes, not a
kernel's share of peak: per round and end 24 bytes (read, gather, write 8) along succ and 48 along pred, r = ceil(log2 n_chains) rounds
each, and one pass over the points (8 bytes read and 8 written, twice that with xy) -- over the time as a fraction of 8 TB/s.  It also
times what the call replaces at its cheapest: the join table and the chain table copied to the host and a point list and a chain table
copied back, with no host walk in between (pageable host memory, as a caller has it) -- a lower bound on the round trip."""
import argparse
import json
import os
import statistics
import sys
import time

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
        for _ in range(16):
            fn()
        t1.record()
        t1.synchronize()
        total += t0.elapsed_time(t1)
        n += 16
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
    out = (torch.empty((n, 2), dtype=torch.int32, device=DEV), torch.empty((m, 4), dtype=torch.int32, device=DEV),
           torch.empty((m, 16), dtype=torch.uint8, device=DEV), torch.empty((m, 16), dtype=torch.uint8, device=DEV),
           torch.empty((n, 2), dtype=torch.float32, device=DEV), torch.empty((2,), dtype=torch.int32, device=DEV))
    joins = lambda: f.chain_joins(points, chains, xy=xy, radius=args.radius, out=join_tab)
    measures = lambda: f.chain_measures(points, chains, xy=xy, out=mea_tab)
    paths = lambda: f.chain_paths(points, chains, join_tab, xy=xy, out=out)
    joins()
    t_path, t_join, t_mea = [], [], []
    for _ in range(args.rounds):                                                # the calls alternate: what drifts, drifts for all
        t_path.append(window(torch, paths, args.window))
        t_join.append(window(torch, joins, args.window))
        t_mea.append(window(torch, measures, args.window))
    t_path, t_join, t_mea = statistics.median(t_path), statistics.median(t_join), statistics.median(t_mea)
    first = [t.cpu().numpy().copy() for t in out]
    paths()
    torch.cuda.synchronize()
    k, q = out[5].cpu().tolist()
    same = all((a == t.cpu().numpy()).all() for a, t in zip(first, out))
    table = out[1][:k].cpu().numpy()
    info = out[3][:k].cpu().numpy().view(cv.SteerableFiltersG2.PATH_INFO_DTYPE).reshape(-1)
    # the cheapest host round trip: tables down, a point list and a table up, nothing done in between
    trips, h_points = [], points.cpu()
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_join, h_chains = join_tab.cpu(), chains.cpu()
        out[0].copy_(h_points)
        out[1].copy_(h_chains)
        torch.cuda.synchronize()
        trips.append(1e3 * (time.perf_counter() - t0))
    tab = join_tab.cpu().numpy().view(cv.SteerableFiltersG2.JOIN_DTYPE).reshape(-1)
    rounds = 0
    while (1 << rounds) < m:
        rounds += 1
    floor = (24.0 + 48.0) * rounds * 2 * m + 2 * 16.0 * n
    blocks = (2 * m + 1023) // 1024
    return {"input": "noise %dx%d" % (args.size, args.size), "radius": args.radius, "points": n, "chains": m,
            "mutual_joins": int(((tab["flags"] & cv.JOIN_MUTUAL) != 0).sum() // 2), "paths": k, "path_points": q,
            "cycles": int(((table[:, 2] & cv.CHAIN_CLOSED) != 0).sum() - ((chains.cpu().numpy()[:, 2] & cv.CHAIN_CLOSED) != 0).sum()),
            "longest_path_members": int(info["n_members"].max()), "longest_path_points": int(table[:, 1].max()),
            "points_per_chain": n / m, "points_per_path": q / max(k, 1), "same_bytes_twice": bool(same),
            "rounds": rounds, "launches": 2 * rounds + 8, "scratch_bytes": 160 * m + 3 * ((4 * (blocks + 1) + 255) // 256 * 256),
            "chain_paths_ms": t_path, "chain_joins_ms": t_join, "chain_measures_ms": t_mea,
            "paths_over_joins": t_path / t_join, "paths_over_measures": t_path / t_mea, "paths_ends_per_ns": 2 * m / (t_path * 1e6),
            "paths_floor_bytes": floor, "paths_floor_frac_of_peak": floor / (t_path * 1e-3) / PEAK,
            "host_round_trip_copies_ms": statistics.median(trips), "paths_over_round_trip_copies": t_path / statistics.median(trips)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paths_probe.json"))
    args = ap.parse_args()
    row = measure(args)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump({"method": "device events around calls repeated over >= %.1f s windows after a warm-up call, the calls alternating in one "
                             "process, %d rounds, medians; the round trip: wall clock around the copies, median of 3" % (args.window, args.rounds),
                   "rows": [row]}, fp, indent=1)


if __name__ == "__main__":
    main()
