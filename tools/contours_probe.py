"""Contour thinning on one MI355X: cvs_nonmax at n = 1 and n = 3 on 4096^2 and 1920x1080 device maps, and
cvs_hysteresis (ms and passes) on thinned 4096^2 maps and on a 1-pixel serpentine across 1024^2.  One process; NMS in timed windows of
>= 1 s after warm-up with device events around each window; hysteresis (which synchronises itself) by wall clock per call; 3 rounds,
medians.

  python tools/contours_probe.py [--window 1.0] [--rounds 3] [--out profiles/contours_probe.json]
  python tools/contours_probe.py --trace-only   # a few calls of each case and nothing else (for rocprofv3 --kernel-trace --stats)

NMS bytes per pixel: theta 4 + n maps x (4 read + 4 written); the fraction is of 8 TB/s."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cvsteer_amd as cv  # noqa: E402

ROOF = 8.0e12
DEV = "cuda:0"


def window(fn, seconds):
    """calls of fn over >= `seconds` of wall time, timed by device events; -> ms per call"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    while True:
        for _ in range(4):
            fn()
        n += 4
        if time.perf_counter() - t0 >= seconds:
            break
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def serpentine(n=1024):
    v = np.zeros((n, n), np.float32)
    for r in range(1, n - 1, 4):
        v[r, 1:n - 1] = 0.5
        turn = n - 2 if (r // 4) % 2 == 0 else 1
        if r + 4 < n - 1:
            v[r + 1:r + 4, turn] = 0.5
    v[1, 1] = 1.0
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contours_probe.json"))
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "method": "NMS: device events around windows of >= %.1f s after one warm-up call, "
           "%d rounds, median; hysteresis: wall clock around each synchronising call (3 calls per round), median" % (args.window, args.rounds),
           "roof_bytes_per_s": ROOF, "nonmax": [], "hysteresis": []}
    cases = {}
    for rows, cols in ((4096, 4096), (1080, 1920)):
        g = torch.Generator(device=DEV).manual_seed(rows)
        img = torch.rand((rows, cols), device=DEV, generator=g)
        f = cv.SteerableFiltersG2(img)
        maps = f.pipeline(img)[5:8]
        outs = [torch.empty_like(m) for m in maps]
        cases[(rows, cols)] = (f, maps, outs)
    if args.trace_only:
        for f, maps, outs in cases.values():
            for n in (1, 3):
                for _ in range(5):
                    f.nonmax(list(maps[:n]), out=outs[:n])
        f, maps, outs = cases[(4096, 4096)]
        thin = f.nonmax(list(maps))
        f.hysteresis(list(thin), 0.1 * float(thin[0].max()), 0.3 * float(thin[0].max()))
        torch.cuda.synchronize()
        return
    for (rows, cols), (f, maps, outs) in cases.items():
        for n in (1, 3):
            ms = [window(lambda: f.nonmax(list(maps[:n]), out=outs[:n]), args.window) for _ in range(args.rounds)]
            med = statistics.median(ms)
            bpp = 4 + 8 * n
            res["nonmax"].append({"rows": rows, "cols": cols, "n": n, "ms_rounds": ms, "ms": med, "bytes_per_pixel": bpp,
                                  "tb_per_s": rows * cols * bpp / (med * 1e-3) / 1e12,
                                  "fraction_of_8tbs": rows * cols * bpp / (med * 1e-3) / ROOF})
            print(res["nonmax"][-1], flush=True)
    f, maps, _ = cases[(4096, 4096)]
    thin = f.nonmax(list(maps))
    hi = max(float(t.max()) for t in thin)
    hyst_cases = [("thinned 4096^2 maps (edges, dark, bright), low / high = 0.05 / 0.2 of the max", f, list(thin), 0.05 * hi, 0.2 * hi),
                  ("thinned 4096^2 edges alone, low / high = 0.05 / 0.2 of the max", f, thin[0], 0.05 * hi, 0.2 * hi)]
    sp = torch.from_numpy(serpentine()).to(DEV)
    fs = cv.SteerableFiltersG2(torch.rand((1024, 1024), device=DEV))
    hyst_cases.append(("1-pixel serpentine across 1024^2, one strong pixel at its end", fs, sp, 0.25, 0.75))
    for name, h, m, low, high in hyst_cases:
        rounds, passes = [], 0
        for _ in range(args.rounds):
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, passes = h.hysteresis(m, low, high, return_passes=True)
                ts.append((time.perf_counter() - t0) * 1e3)
            rounds.append(statistics.median(ts))
        res["hysteresis"].append({"case": name, "ms_rounds": rounds, "ms": statistics.median(rounds), "passes": passes})
        print(res["hysteresis"][-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(res, fo, indent=1)


if __name__ == "__main__":
    main()
