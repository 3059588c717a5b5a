"""Contour components on one MI355X: cvs_label, cvs_contour_prune (n = 1, 3) and cvs_contour_points at 4096^2 and
1920x1080 on (a) the hysteresis masks of the thinned pipeline maps of a noise image (uint8) and (b) a 0.45-density random mask (f32),
with cvs_hysteresis on the same input for scale.  One process; every call synchronises itself, so: wall clock around calls repeated
over windows of >= 1 s after a warm-up call, 3 rounds, medians.

  python tools/components_probe.py [--window 1.0] [--rounds 3] [--out profiles/components_probe.json]
  python tools/components_probe.py --trace-only          # a few cvs_label calls and nothing else (for rocprofv3 --kernel-trace --stats)
  python tools/components_probe.py --check-trace X.csv   # the kernel list per cvs_label call from that run's kernel trace ->
                                                         # profiles/components_kernel_trace.csv; fails unless serpentine and random agree

Bytes the labelling must move: the mask read (1 or 4 B/pixel) + the labels written (4): the fraction is of 8 TB/s, no target."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8.0e12
DEV = "cuda:0"
TRACE_CALLS = 3


def serpentine(n=1024):
    v = np.zeros((n, n), np.float32)
    for r in range(1, n - 1, 4):
        v[r, 1:n - 1] = 0.5
        turn = n - 2 if (r // 4) % 2 == 0 else 1
        if r + 4 < n - 1:
            v[r + 1:r + 4, turn] = 0.5
    v[1, 1] = 1.0
    return v


def window(fn, seconds):
    """synchronising calls of fn over >= `seconds` of wall time -> ms per call"""
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e3 * dt / n


def check_trace(path, out):
    """kernel names per cvs_label call, in launch order: the TRACE_CALLS serpentine calls, one prune (the separator), the random ones"""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ours = [(r["Kernel_Name"].split("(")[0].replace("void cvs::", "").replace("cvs::", ""), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            for r in rows if any(s in r["Kernel_Name"] for s in ("k_cc_", "k_scan_", "k_prune_", "k_zero_ints"))]
    cut = next(i for i, (k, _) in enumerate(ours) if k.startswith("k_zero_ints"))
    end = max(i for i, (k, _) in enumerate(ours) if k.startswith("k_prune_emit"))
    phases = {"serpentine 1024^2": ours[:cut], "random 0.45 1024^2": ours[end + 1:]}
    lists = {}
    with open(out, "w") as fo:
        fo.write("# rocprofv3 --kernel-trace --stats -- python tools/components_probe.py --trace-only, one MI355X; durations in us (device timestamps)\n")
        fo.write("# %d cvs_label calls per mask after one warm-up call each; kernels in launch order\n" % TRACE_CALLS)
        fo.write("mask,call,kernel,us\n")
        for name, ks in phases.items():
            starts = [i for i, (k, _) in enumerate(ks) if k.startswith("k_cc_tiles")]
            calls = [ks[a:b] for a, b in zip(starts, starts[1:] + [len(ks)])][-TRACE_CALLS:]
            lists[name] = [[k for k, _ in c] for c in calls]
            for j, c in enumerate(calls):
                for k, us in c:
                    fo.write("%s,%d,%s,%.2f\n" % (name, j, k, us))
    a, b = lists.values()
    print("kernels per cvs_label call:", a[0])
    assert len(a) == len(b) == TRACE_CALLS and all(x == a[0] for x in a + b), lists
    print("launch list identical for the serpentine and the random mask: %d kernels per call" % len(a[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_probe.json"))
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--check-trace", default=None)
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "components_kernel_trace.csv"))
    args = ap.parse_args()
    if args.check_trace:
        return check_trace(args.check_trace, args.trace_out)
    import torch
    import cvsteer_amd as cv
    if args.trace_only:
        f = cv.SteerableFiltersG2(torch.rand((1024, 1024), device=DEV))
        sp = torch.from_numpy(serpentine()).to(DEV)
        rnd = (torch.rand((1024, 1024), device=DEV) < 0.45).float()
        for _ in range(TRACE_CALLS + 1):
            f.label(sp)
        f.prune(rnd, 8)   # the separator of the two lists in the trace
        for _ in range(TRACE_CALLS + 1):
            f.label(rnd)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "method": "wall clock around synchronising calls repeated over windows of >= %.1f s after one "
           "warm-up call, %d rounds, median" % (args.window, args.rounds), "roof_bytes_per_s": ROOF, "cases": []}
    for rows, cols in ((4096, 4096), (1080, 1920)):
        g = torch.Generator(device=DEV).manual_seed(rows)
        img = torch.rand((rows, cols), device=DEV, generator=g)
        f = cv.SteerableFiltersG2(img)
        thin = f.nonmax(f.pipeline(img)[5:8])
        hi = max(float(t.max()) for t in thin)
        low, high = 0.05 * hi, 0.2 * hi
        linked = f.hysteresis(list(thin), low, high)
        rnd = [(torch.rand((rows, cols), device=DEV, generator=g) < 0.45).float() for _ in range(3)]
        for name, masks, weights, mask_bytes in (("hysteresis masks of the thinned maps of a noise image (uint8)", list(linked), list(thin), 1),
                                                 ("random mask, density 0.45 (f32)", rnd, None, 4)):
            labels, count = f.label(masks[0])
            npts = int((labels != 0).sum())
            outs = [torch.empty((rows, cols), dtype=torch.uint8, device=DEV) for _ in range(3)]
            ops = [("label", lambda: f.label(masks[0], out=labels), mask_bytes + 4),
                   ("prune n=1 (min_area 8)", lambda: f.prune(masks[0], 8, out=outs[0]), mask_bytes + 1),
                   ("prune n=3 (min_area 8)", lambda: f.prune(masks, 8, out=outs), 3 * (mask_bytes + 1)),
                   ("contour_points", lambda: f.contour_points(labels), 4 + 12.0 * npts / (rows * cols))]
            if weights is not None:
                ops.append(("prune n=3 (min_area 8, min_peak = high, weighted)", lambda: f.prune(masks, 8, weight=weights, min_peak=high, out=outs),
                            3 * (mask_bytes + 4 + 1)))
                ops.append(("hysteresis n=1 (for scale)", lambda: f.hysteresis(weights[0], low, high), None))
                ops.append(("hysteresis n=3 (for scale)", lambda: f.hysteresis(weights, low, high), None))
            for op, fn, bpp in ops:
                ms = [window(fn, args.window) for _ in range(args.rounds)]
                med = statistics.median(ms)
                rec = {"rows": rows, "cols": cols, "input": name, "components": count, "labelled_pixels": npts, "op": op, "ms_rounds": ms, "ms": med}
                if bpp is not None:
                    rec.update({"bytes_per_pixel": bpp, "fraction_of_8tbs": rows * cols * bpp / (med * 1e-3) / ROOF})
                res["cases"].append(rec)
                print(rec, flush=True)
    sp = torch.from_numpy(serpentine()).to(DEV)
    fs = cv.SteerableFiltersG2(torch.rand((1024, 1024), device=DEV))
    for op, fn in (("label", lambda: fs.label(sp)), ("hysteresis", lambda: fs.hysteresis(sp, 0.25, 0.75))):
        ms = [window(fn, args.window) for _ in range(args.rounds)]
        res["cases"].append({"rows": 1024, "cols": 1024, "input": "1-pixel serpentine", "op": op, "ms_rounds": ms, "ms": statistics.median(ms)})
        print(res["cases"][-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(res, fo, indent=1)


if __name__ == "__main__":
    main()
