"""Contour chains on one MI355X: cvs_contour_chains on (a) the thinned contours() masks of a noise image at 4096^2 and
1920x1080 (uint8), (b) the 1024^2 one-pixel serpentine and (c) a 0.45-density random mask at 1080p (f32).  Beside them, in the same
process: label + contour_points of the same mask -- the raster-ordered listing that existed before -- and, for the 1080p thinned mask, the
host walk of tests/chains_model.py, which is what callers did with that listing.  One process; every call synchronises itself, so: wall
clock around calls repeated over windows of >= 1 s after a warm-up call, 3 rounds, medians.

  python tools/chains_probe.py [--window 1.0] [--rounds 3] [--out profiles/chains_probe.json]
  python tools/chains_probe.py --trace-only          # a few calls on the serpentine, then on a mask of many short chains, and nothing else
                                                     # (for rocprofv3 --kernel-trace --stats)
  python tools/chains_probe.py --check-trace X.csv   # the kernel list per call from that run's kernel trace -> profiles/chains_kernel_trace.csv;
                                                     # fails unless the two lists differ in the number of k_ch_jump rounds only

Bytes per pixel, counted from the loads and stores of the kernels: the mask (1 or 4) + 32 over the planes (links 2 written and 10 read,
parent and flags 8 written, parent 4 read, arc bases 4 written and 4 read) + per arc A / pixels x (16 built + 24 per jump round + 72 in
heads, scans and emit, gathers counted once)."""
import argparse
import csv
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

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


def arcs_of(table, pts):
    """directed links + pseudo arcs of the isolated pixels, from the lists: an open chain of n points has n - 1 links, a closed one n"""
    t = table.cpu().numpy() if hasattr(table, "cpu") else table
    closed = (t[:, 2] & 1) != 0
    links = int((t[:, 1] - 1)[~closed].sum() + t[:, 1][closed].sum())
    return 2 * links + int(((t[:, 1] == 1) & ~closed).sum())


def bytes_per_pixel(mask_bytes, arcs, npix):
    rounds = max(0, math.ceil(math.log2(arcs))) if arcs > 1 else 0
    return mask_bytes + 32 + arcs / npix * (16 + 24 * rounds + 72)


def check_trace(path, out):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ours = [(r["Kernel_Name"].split("(")[0].replace("void cvs::", "").replace("cvs::", ""), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            for r in rows if any(s in r["Kernel_Name"] for s in ("k_ch_", "k_cc_", "k_scan_", "k_zero_ints", "k_prune_"))]
    cut = next(i for i, (k, _) in enumerate(ours) if k.startswith("k_prune_emit"))   # the separator: one prune between the two masks
    phases = {"serpentine 1024^2": ours[:cut], "isolated pixels 1024^2": ours[cut + 1:]}
    lists = {}
    with open(out, "w") as fo:
        fo.write("# rocprofv3 --kernel-trace --stats -- python tools/chains_probe.py --trace-only, one MI355X; durations in us (device timestamps)\n")
        fo.write("# %d cvs_contour_chains calls (sizing call + filling call each) per mask after one warm-up; kernels in launch order\n" % TRACE_CALLS)
        fo.write("mask,call,kernel,us\n")
        for name, ks in phases.items():
            starts = [i for i, (k, _) in enumerate(ks) if k.startswith("k_ch_arc_count")]
            firsts = [max(j for j in range(s) if ks[j][0].startswith("k_zero_ints")) for s in starts]
            calls = [ks[a:b] for a, b in zip(firsts, firsts[1:] + [len(ks)])][-TRACE_CALLS:]
            lists[name] = [[k for k, _ in c] for c in calls]
            for j, c in enumerate(calls):
                for k, us in c:
                    fo.write("%s,%d,%s,%.2f\n" % (name, j, k, us))
    strip = lambda ks: [k for k in ks if not k.startswith("k_ch_jump")]
    a, b = lists.values()
    print("kernels per filling call (serpentine):", a[0])
    print("jump rounds: %d (serpentine), %d (isolated pixels)" % (sum(k.startswith("k_ch_jump") for k in a[0]), sum(k.startswith("k_ch_jump") for k in b[0])))
    assert all(x == a[0] for x in a) and all(x == b[0] for x in b) and strip(a[0]) == strip(b[0]), lists


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chains_probe.json"))
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--check-trace", default=None)
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "chains_kernel_trace.csv"))
    args = ap.parse_args()
    if args.check_trace:
        return check_trace(args.check_trace, args.trace_out)
    import torch
    import cvsteer_amd as cv
    sp = torch.from_numpy(serpentine()).to(DEV)
    if args.trace_only:
        f = cv.SteerableFiltersG2(torch.rand((1024, 1024), device=DEV))
        dots = torch.zeros((1024, 1024), device=DEV)
        dots[::2, ::2] = 1.0   # many chains of one point each
        for _ in range(TRACE_CALLS + 1):
            f.contour_chains(sp)
        f.prune(dots, 8)   # the separator of the two lists in the trace
        for _ in range(TRACE_CALLS + 1):
            f.contour_chains(dots)
        torch.cuda.synchronize()
        return
    import chains_model
    res = {"device": torch.cuda.get_device_name(0), "method": "wall clock around synchronising calls repeated over windows of >= %.1f s after one "
           "warm-up call, %d rounds, median" % (args.window, args.rounds), "cases": []}

    def run(f, name, mask, mask_bytes, host_walk=False):
        rows, cols = mask.shape
        pts, table = f.contour_chains(mask)
        arcs = arcs_of(table, pts)
        labels, count = f.label(mask)
        ops = [("contour_chains", lambda: f.contour_chains(mask)),
               ("label + contour_points (raster order, for scale)", lambda: f.contour_points(f.label(mask, out=labels)[0]))]
        for op, fn in ops:
            ms = [window(fn, args.window) for _ in range(args.rounds)]
            rec = {"rows": rows, "cols": cols, "input": name, "op": op, "chains": len(table), "points": len(pts), "arcs": arcs,
                   "components": count, "ms_rounds": ms, "ms": statistics.median(ms)}
            if op == "contour_chains":
                rec["bytes_per_pixel"] = bytes_per_pixel(mask_bytes, arcs, rows * cols)
            res["cases"].append(rec)
            print(rec, flush=True)
        if host_walk:
            host = mask.cpu().numpy()
            ms = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                chains_model.chains(host)
                ms.append(1e3 * (time.perf_counter() - t0))
            res["cases"].append({"rows": rows, "cols": cols, "input": name, "op": "host walk (tests/chains_model.py)", "ms_rounds": ms,
                                 "ms": statistics.median(ms)})
            print(res["cases"][-1], flush=True)

    for rows, cols in ((4096, 4096), (1080, 1920)):
        g = torch.Generator(device=DEV).manual_seed(rows)
        img = torch.rand((rows, cols), device=DEV, generator=g)
        f = cv.SteerableFiltersG2(img)
        thin = f.nonmax(f.pipeline(img)[5:8])
        hi = max(float(t.max()) for t in thin)
        masks = f.contours(img, 0.05 * hi, 0.2 * hi)
        run(f, "thinned contours() edges mask of a noise image (uint8)", masks[0], 1, host_walk=rows == 1080)
        if rows == 1080:
            run(f, "random mask, density 0.45 (f32)", (torch.rand((rows, cols), device=DEV, generator=g) < 0.45).float(), 4)
    run(cv.SteerableFiltersG2(torch.rand((1024, 1024), device=DEV)), "1-pixel serpentine (f32)", sp, 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(res, fo, indent=1)


if __name__ == "__main__":
    main()
