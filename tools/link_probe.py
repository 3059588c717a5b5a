"""The contour chain on the batch axis on one MI355X ("Contour batches"): the new path against the existing entry
points it replaces, ALTERNATED in the same process -- link against hysteresis + prune on the thinned maps of a noise image (4096^2, n = 3;
32 x 3 planes of 1080p), on the 1024^2 serpentine and on a 0.45-density random plane; contours_batch against the per-frame contours() loop for
32 x 1080p.  One process; wall clock around calls followed by a synchronisation, repeated over windows of >= 1 s after a warm-up call, 3
rounds, medians.

  python tools/link_probe.py [--window 1.0] [--rounds 3] [--out profiles/link_probe.json]
  python tools/link_probe.py --trace-only          # a few link calls per mask and nothing else (for rocprofv3 --kernel-trace --stats)
  python tools/link_probe.py --check-trace X.csv   # the kernel list per link call from that run's kernel trace ->
                                                   # profiles/link_kernel_trace.csv; fails unless serpentine, random and empty agree

Bytes the link must move per pixel: the plane read (4) + the mask written (1); the fraction is of 8 TB/s, no target."""
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
LINK_KERNELS = ("k_link_tiles", "k_link_borders", "k_link_stats", "k_link_emit", "k_link_table")


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
    """calls of fn, each followed by a synchronisation, over >= `seconds` of wall time -> ms per call"""
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e3 * dt / n


def alternate(pairs, seconds, rounds):
    """[(name, fn)] -> {name: (median ms, [ms per round])}, the functions taking turns inside every round"""
    ms = {name: [] for name, _ in pairs}
    for _ in range(rounds):
        for name, fn in pairs:
            ms[name].append(window(fn, seconds))
    return {name: (statistics.median(v), v) for name, v in ms.items()}


def check_trace(path, out):
    """kernel names per link call, in launch order; the three phases are separated by one k_hyst_classify each (a hysteresis call)"""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ours = [(r["Kernel_Name"].split("(")[0].replace("void cvs::", "").replace("cvs::", ""), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            for r in rows if any(s in r["Kernel_Name"] for s in LINK_KERNELS + ("k_hyst_classify",))]
    phases, cur = [], []
    for k, us in ours:
        if k.startswith("k_hyst_classify"):
            phases.append(cur)
            cur = []
        else:
            cur.append((k, us))
    phases.append(cur)
    names = ("serpentine 1024^2", "random 0.45 1024^2", "empty 1024^2")
    assert len(phases) == len(names), [len(p) for p in phases]
    lists = {}
    with open(out, "w") as fo:
        fo.write("# rocprofv3 --kernel-trace --stats -- python tools/link_probe.py --trace-only, one MI355X; durations in us (device timestamps)\n")
        fo.write("# %d link calls per plane after one warm-up call each; kernels in launch order\n" % TRACE_CALLS)
        fo.write("plane,call,kernel,us\n")
        for name, ks in zip(names, phases):
            starts = [i for i, (k, _) in enumerate(ks) if k.startswith("k_link_tiles")]
            calls = [ks[a:b] for a, b in zip(starts, starts[1:] + [len(ks)])][-TRACE_CALLS:]
            lists[name] = [[k for k, _ in c] for c in calls]
            for j, c in enumerate(calls):
                for k, us in c:
                    fo.write("%s,%d,%s,%.2f\n" % (name, j, k, us))
    first = lists[names[0]][0]
    print("kernels per link call:", first)
    assert all(len(v) == TRACE_CALLS and all(x == first for x in v) for v in lists.values()), lists
    print("launch list identical for the serpentine, the random plane and the empty plane: %d kernels per call" % len(first))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_probe.json"))
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--check-trace", default=None)
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "link_kernel_trace.csv"))
    args = ap.parse_args()
    if args.check_trace:
        return check_trace(args.check_trace, args.trace_out)
    import torch
    import cvsteer_amd as cv
    sp = torch.from_numpy(serpentine()).to(DEV)
    rnd = torch.rand((1024, 1024), device=DEV) * (torch.rand((1024, 1024), device=DEV) < 0.45)
    fs = cv.SteerableFiltersG2(torch.rand((1024, 1024), device=DEV))
    if args.trace_only:
        out = torch.empty((1024, 1024), dtype=torch.uint8, device=DEV)
        for k, plane in enumerate((sp, rnd, torch.zeros((1024, 1024), device=DEV))):
            if k:
                fs.hysteresis(plane, 0.25, 0.75)   # the separator of the lists in the trace
            for _ in range(TRACE_CALLS + 1):
                fs.link(plane, 0.25, 0.75, 8, out=out)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "method": "old and new path alternated in one process; wall clock around calls + a synchronisation, "
           "repeated over windows of >= %.1f s after one warm-up call, %d rounds, median" % (args.window, args.rounds),
           "roof_bytes_per_s": ROOF, "cases": []}

    def record(what, rows, cols, n, timed, bpp=None):
        for name, (med, ms) in timed.items():
            rec = {"what": what, "rows": rows, "cols": cols, "planes": n, "op": name, "ms_rounds": ms, "ms": med}
            if bpp is not None and name == "link":
                rec.update({"bytes_per_pixel": bpp, "fraction_of_8tbs": n * rows * cols * bpp / (med * 1e-3) / ROOF})
            res["cases"].append(rec)
            print(rec, flush=True)

    # 1. link against hysteresis + prune on thinned maps
    for rows, cols, frames in ((4096, 4096, 1), (1080, 1920, 32)):
        g = torch.Generator(device=DEV).manual_seed(rows)
        imgs = torch.rand((frames, rows, cols), device=DEV, generator=g)
        f = cv.SteerableFiltersG2(None)
        maps = f.pipeline_batch(imgs, outputs=(5, 6, 7))
        thin = f.nonmax_batch(maps).view(frames * 3, rows, cols)
        del maps
        hi = float(thin.max())
        low, high = 0.05 * hi, 0.2 * hi
        planes = list(thin)
        out = torch.empty((frames * 3, rows, cols), dtype=torch.uint8, device=DEV)
        outs = list(out)
        old = lambda: f.prune(f.hysteresis(planes, low, high), 8, weight=planes, min_peak=high, out=outs)
        new = lambda: f.link(thin, low, high, 8, high, out=out)
        record("thinned maps of noise images", rows, cols, frames * 3,
               alternate([("hysteresis + prune", old), ("link", new)], args.window, args.rounds), bpp=5)
        del f, thin, planes, out, outs, imgs
        torch.cuda.empty_cache()
    # 2. the serpentine and the random plane
    o1 = torch.empty((1024, 1024), dtype=torch.uint8, device=DEV)
    for what, plane in (("1-pixel serpentine", sp), ("random plane, density 0.45", rnd)):
        old = lambda: fs.prune(fs.hysteresis(plane, 0.25, 0.75), 8, weight=plane, min_peak=0.0, out=o1)
        new = lambda: fs.link(plane, 0.25, 0.75, 8, 0.0, out=o1)
        record(what, 1024, 1024, 1, alternate([("hysteresis + prune", old), ("link", new)], args.window, args.rounds), bpp=5)
    # 3. contours_batch against the per-frame loop
    rows, cols, frames = 1080, 1920, 32
    imgs = torch.rand((frames, rows, cols), device=DEV)
    fb, fl = cv.SteerableFiltersG2(None), cv.SteerableFiltersG2(None)
    thin = fl.nonmax(fl.pipeline(imgs[0])[5:8])
    hi = max(float(t.max()) for t in thin)
    low, high = 0.05 * hi, 0.2 * hi
    loop = lambda: [fl.contours(imgs[i], low, high, 8, 0.0) for i in range(frames)]
    batch = lambda: fb.contours_batch(imgs, low, high, 8, 0.0)
    record("contours of 32 frames", rows, cols, frames * 3, alternate([("per-frame contours() loop", loop), ("contours_batch", batch)], args.window, args.rounds))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(res, fo, indent=1)


if __name__ == "__main__":
    main()
