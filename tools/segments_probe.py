"""Contour segments on one MI355X: how cvs_polyline_segments is timed, and against what.

Inputs, all device arrays: the chains of the thinned contours() edges of a 4096^2 noise frame, their polylines at eps = 1.0 and the refined
positions and strengths of chain_refine on the un-thinned edges map.  The yardstick is cvs_chain_measures on the same point list and chain
table with the same xy and strength: the same arrays cross the memory system once, with the same split into waves and workgroups; the
segments read each point of a span twice (the second pass, which L2 should serve) and a vertex's point in both of its spans, and write
128 bytes per vertex where the measures write 40 per chain.  Neither call synchronises, so each is timed by DEVICE EVENTS around calls
repeated over windows of >= 1 s after a warm-up call, the two calls alternating within a round, 3 rounds, medians.

Every measurement runs in a process of its own.  Where the twin of `make -C cvsteer_amd/csrc segwave` exists
(tools/libcvsteer_hip_segwave.so: the same kernels with a whole wave per span of up to 256 points, where the library takes 16 lanes), the
library and the twin are measured in turn, twice each, so that the two can be compared within one run.

  python tools/segments_probe.py [--window 1.0] [--rounds 3] [--size 4096] [--out profiles/segments_probe.json]

The table prints ms per call and points per ns for both calls, the ratio of the two, and the bytes that must move at least over the time as
a fraction of 8 TB/s -- a floor from shapes, not a kernel's share of peak: for the segments 12 bytes per point (xy and strength; the integer
point list is read for the origin of a span only), 12 per vertex read (index, origin) and 128 written, 32 per chain (the two tables); for
the measures 12 bytes per point + 16 + 40 per chain."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
PEAK = 8e12   # bytes per second
TWIN = os.path.join(ROOT, "tools", "libcvsteer_hip_segwave.so")


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
    """one process, one library (CVSTEER_HIP_LIB or the product's): a row of the table"""
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
    _, polylines, index = f.chain_polylines(points, chains, 1.0, return_index=True)
    xy, strength = f.chain_refine(points, edges)
    n, m, v = int(points.shape[0]), int(chains.shape[0]), int(index.shape[0])
    seg_tab = torch.empty((v, 128), dtype=torch.uint8, device=DEV)
    mea_tab = torch.empty((m, 40), dtype=torch.uint8, device=DEV)
    segments = lambda: f.polyline_segments(points, chains, polylines, index, xy=xy, strength=strength, out=seg_tab)
    measures = lambda: f.chain_measures(points, chains, strength=strength, xy=xy, out=mea_tab)
    t_seg, t_mea = [], []
    for _ in range(args.rounds):                                                # the two alternate: what drifts, drifts for both
        t_seg.append(window(torch, segments, args.window))
        t_mea.append(window(torch, measures, args.window))
    t_seg, t_mea = statistics.median(t_seg), statistics.median(t_mea)
    seg = seg_tab.cpu().numpy().view(cv.SteerableFiltersG2.SEGMENT_DTYPE).reshape(-1)
    fitted = seg[seg["count"] >= 2]
    return {"library": args.child, "input": "noise %dx%d" % (args.size, args.size), "points": n, "chains": m, "vertices": v,
            "spans": int(len(fitted)), "span_points": int(fitted["count"].sum()), "longest_span": int(seg["count"].max()) if v else 0,
            "spans_over_256_points": int((seg["count"] > 256).sum()), "degenerate": int(((seg["flags"] & cv.SEG_DEGENERATE) != 0).sum()),
            "polyline_segments_ms": t_seg, "chain_measures_ms": t_mea, "segments_over_measures": t_seg / t_mea,
            "segments_points_per_ns": n / (t_seg * 1e6), "measures_points_per_ns": n / (t_mea * 1e6),
            "segments_floor_frac_of_peak": (12.0 * n + 140.0 * v + 32.0 * m) / (t_seg * 1e-3) / PEAK,
            "measures_floor_frac_of_peak": (12.0 * n + 56.0 * m) / (t_mea * 1e-3) / PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments_probe.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("ROW " + json.dumps(measure(args)))
        return
    runs = [("16 lanes per span (the library)", None)]
    if os.path.exists(TWIN):
        runs = (runs + [("64 lanes per span (segwave twin)", TWIN)]) * 2
    rows = []
    for label, so in runs:                                                      # a fresh process each: this one never opens the GPU
        env = dict(os.environ)
        env.pop("CVSTEER_HIP_LIB", None)
        if so:
            env["CVSTEER_HIP_LIB"] = so
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", label, "--window", str(args.window), "--rounds",
                              str(args.rounds), "--size", str(args.size)], env=env, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            sys.exit("the measurement of '%s' failed (%d):\n%s%s" % (label, out.returncode, out.stdout, out.stderr))
        row = json.loads([line for line in out.stdout.splitlines() if line.startswith("ROW ")][-1][4:])
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump({"method": "device events around calls repeated over >= %.1f s windows after a warm-up call, the two calls alternating, "
                             "%d rounds, medians; one process per row, the libraries in turn" % (args.window, args.rounds), "rows": rows},
                  fp, indent=1)


if __name__ == "__main__":
    main()
