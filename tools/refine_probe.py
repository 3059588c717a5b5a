"""Contour edgels on one MI355X: how cvs_chain_refine and cvs_chain_measures are to be timed.  No figure from this
tool is in the record yet; profiles/refine_probe.json is what a run writes.

Inputs, all device arrays: the chains of the thinned contours() edges of a noise image at 4096^2 and at 1920x1080 (the un-thinned edges map
of the same pipeline call is the map, the object's own theta the orientation), and one chain of 262144 points along a sine on a 256 x
262144 noise map with a random theta plane (the workgroup kernel of the measures).  Neither call synchronises, so: the stream is
synchronised around calls repeated over windows of >= 1 s after a warm-up call, 3 rounds, medians.

  python tools/refine_probe.py [--window 1.0] [--rounds 3] [--out profiles/refine_probe.json]

Bytes per point, counted from the kernels' loads and stores: refine 8 (the point) + 12 (xy, strength) + the gathers -- 40 if no line were
shared, far fewer where consecutive points are neighbours; measures 8 (or 16 with xy) + 4 for each of the point and its successor, which
the caches serve once, + 40 per chain.  The table prints ms per call, points per ns and, with the bytes that must move at least (20 and
12 per point), the fraction of 8 TB/s."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
PEAK = 8e12   # bytes per second


def window(fn, seconds):
    """fn repeated over >= `seconds` of wall time between two synchronisations -> ms per call"""
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        for _ in range(16):
            fn()
        n += 16
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e3 * dt / n


def noise_case(cv, torch, rows, cols):
    img = torch.rand((rows, cols), device=DEV) * 255
    f = cv.SteerableFiltersG2(img)
    edges = f.pipeline(img)[5]
    hi = float(f.nonmax(edges).max())
    mask = f.contours(img, 0.05 * hi, 0.2 * hi)[0]
    points, chains = f.contour_chains(mask)
    return f, edges, None, points, chains


def sine_case(cv, torch, n=262144, rows=256):
    s = np.arange(n)
    pts = np.stack([s, np.rint(rows / 2 + 100 * np.sin(s / 150.0)).astype(np.int64)], axis=1).astype(np.int32)
    f = cv.SteerableFiltersG2(torch.zeros((rows, n), device=DEV))
    m = torch.rand((rows, n), device=DEV)
    theta = (torch.rand((rows, n), device=DEV) * 2 - 1) * float(np.pi)
    return f, m, theta, torch.from_numpy(pts).to(DEV), torch.tensor([[0, n, 0, 0]], dtype=torch.int32, device=DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_probe.json"))
    args = ap.parse_args()
    import torch
    import cvsteer_amd as cv
    cases = {"noise 4096x4096": lambda: noise_case(cv, torch, 4096, 4096), "noise 1080x1920": lambda: noise_case(cv, torch, 1080, 1920),
             "one chain of 262144 points": lambda: sine_case(cv, torch)}
    rows = []
    for name, make in cases.items():
        f, m, theta, points, chains = make()
        n, k = int(points.shape[0]), int(chains.shape[0])
        xy = torch.empty((n, 2), dtype=torch.float32, device=DEV)
        st = torch.empty((n,), dtype=torch.float32, device=DEV)
        tab = torch.empty((k, 40), dtype=torch.uint8, device=DEV)
        refine = lambda: f.chain_refine(points, m, theta, out=(xy, st))
        measure = lambda: f.chain_measures(points, chains, strength=st, xy=xy, out=tab)
        t_ref = statistics.median(window(refine, args.window) for _ in range(args.rounds))
        t_mea = statistics.median(window(measure, args.window) for _ in range(args.rounds))
        row = {"input": name, "points": n, "chains": k, "longest_chain": int(chains[:, 1].max()) if k else 0,
               "chain_refine_ms": t_ref, "chain_measures_ms": t_mea,
               "refine_points_per_ns": n / (t_ref * 1e6), "measures_points_per_ns": n / (t_mea * 1e6),
               "refine_frac_of_peak": 20.0 * n / (t_ref * 1e-3) / PEAK, "measures_frac_of_peak": (12.0 * n + 40.0 * k) / (t_mea * 1e-3) / PEAK}
        print(json.dumps(row))
        rows.append(row)
    with open(args.out, "w") as fp:
        json.dump({"method": "stream synchronised around >= %.1f s windows after a warm-up call, %d rounds, medians" % (args.window, args.rounds),
                   "rows": rows}, fp, indent=1)


if __name__ == "__main__":
    main()
