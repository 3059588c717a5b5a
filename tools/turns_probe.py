"""Contour turns on one MI355X: how cvs_chain_turns is timed, and against what.

Inputs, all device arrays: the chains of the thinned contours() edges of a 4096^2 noise frame and the refined positions of chain_refine on
the un-thinned edges map.  The yardstick is cvs_chain_measures on the same point list and chain table with the same xy: the same arrays
cross the memory system once; the turns read every point's window (served by LDS and L2) and write 32 bytes per POINT where the measures
write 40 per chain.  Neither call synchronises, so each is timed by DEVICE EVENTS around calls repeated over windows of >= 1 s after a
warm-up call, the calls alternating within a round, 3 rounds, medians, all in ONE process.  Nothing is fixed in advance: the probe records
what it finds.

  python tools/turns_probe.py [--window 1.0] [--rounds 3] [--size 4096] [--out profiles/turns_probe.json]

The row holds ms per call for the turns with and without the summary and for the measures, the ratio to the measures, points per ns, and
the bytes that must move at least per point -- a floor from shapes, not a kernel's share of peak: 8 bytes of xy read and 32 of record
written by the first launch, the record read and 4 bytes of it written by the second (32 + 4), the record read once more by the summary
(32, and 16 + 16 per chain for the table entry and the summary) -- over the time as a fraction of 8 TB/s."""
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
    turn_tab = torch.empty((n, 32), dtype=torch.uint8, device=DEV)
    sum_tab = torch.empty((m, 16), dtype=torch.uint8, device=DEV)
    mea_tab = torch.empty((m, 40), dtype=torch.uint8, device=DEV)
    turns = lambda: f.chain_turns(points, chains, xy=xy, radius=args.radius, out=turn_tab)
    turns_sum = lambda: f.chain_turns(points, chains, xy=xy, radius=args.radius, summary=True, out=(turn_tab, sum_tab))
    measures = lambda: f.chain_measures(points, chains, xy=xy, out=mea_tab)
    t_turn, t_sum, t_mea = [], [], []
    for _ in range(args.rounds):                                                # the calls alternate: what drifts, drifts for all
        t_turn.append(window(torch, turns, args.window))
        t_mea.append(window(torch, measures, args.window))
        t_sum.append(window(torch, turns_sum, args.window))
    t_turn, t_sum, t_mea = statistics.median(t_turn), statistics.median(t_sum), statistics.median(t_mea)
    tab = turn_tab.cpu().numpy().view(cv.SteerableFiltersG2.TURN_DTYPE).reshape(-1)
    lengths = chains[:, 1].cpu().numpy()
    eligible = (tab["flags"] & (cv.TURN_END | cv.TURN_DEGENERATE | cv.TURN_SHORT | cv.TURN_NO_CHAIN)) == 0
    bytes_turns, bytes_sum = 8.0 + 32.0 + 36.0, 8.0 + 32.0 + 36.0 + 32.0
    return {"input": "noise %dx%d" % (args.size, args.size), "radius": args.radius, "points": n, "chains": m,
            "mean_chain_points": float(lengths.mean()) if m else 0.0, "longest_chain": int(lengths.max()) if m else 0,
            "chains_over_256_points": int((lengths > 256).sum()), "eligible": int(eligible.sum()),
            "corners": int(((tab["flags"] & cv.TURN_CORNER) != 0).sum()), "degenerate": int(((tab["flags"] & cv.TURN_DEGENERATE) != 0).sum()),
            "chain_turns_ms": t_turn, "chain_turns_with_summary_ms": t_sum, "chain_measures_ms": t_mea,
            "turns_over_measures": t_turn / t_mea, "turns_with_summary_over_measures": t_sum / t_mea,
            "turns_points_per_ns": n / (t_turn * 1e6), "measures_points_per_ns": n / (t_mea * 1e6),
            "turns_bytes_per_point": bytes_turns, "turns_with_summary_bytes_per_point": bytes_sum + 32.0 * m / max(n, 1),
            "turns_floor_frac_of_peak": bytes_turns * n / (t_turn * 1e-3) / PEAK,
            "turns_with_summary_floor_frac_of_peak": (bytes_sum * n + 32.0 * m) / (t_sum * 1e-3) / PEAK,
            "measures_floor_frac_of_peak": (8.0 * n + 56.0 * m) / (t_mea * 1e-3) / PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "turns_probe.json"))
    args = ap.parse_args()
    row = measure(args)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump({"method": "device events around calls repeated over >= %.1f s windows after a warm-up call, the calls alternating in one "
                             "process, %d rounds, medians" % (args.window, args.rounds), "rows": [row]}, fp, indent=1)


if __name__ == "__main__":
    main()
