"""Contour polylines on one MI355X: cvs_chain_polylines (device arrays, eps = 1) on the chains of (a) the thinned
contours() edge masks of a noise image at 4096^2 and 1920x1080 and (b) the 1024^2 one-pixel serpentine, one chain of half a million points.
The chains come from contour_chains on the device and stay there.  Beside each: the host walk a caller would otherwise do -- host_polylines
below, the contract's split rule with numpy int64 over each segment -- on the same lists (timed once; on the leading chains up to
--host-points points, at least one whole chain; the count is in the row), its vertices compared with the device's; and on the leading
chains up to 20000 points the plain Python model of tests/polyline_model.py is compared too.
One process; every call synchronises itself, so: wall clock around calls repeated over windows of >= 1 s after a warm-up call, 3 rounds,
medians.

  python tools/polylines_probe.py [--window 1.0] [--rounds 3] [--eps 1.0] [--host-points 200000] [--out profiles/polylines_probe.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"


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


def host_polylines(points, table, eps):
    """the split rule of include/cvsteer_hip.h on the host: per segment the values as one int64 numpy expression, np.argmax for the smallest
    index with the largest value; returns the vertices"""
    e2 = np.float64(np.float32(eps)) ** 2
    out = []
    for start, length, flags, _ in table.tolist():
        p = points[start:start + length].astype(np.int64)
        if length <= 2:
            out.append(p)
            continue
        q = np.concatenate([p, p[:1]]) if flags & 1 else p
        keep = np.zeros(len(q), bool)
        keep[0] = keep[-1] = True
        stack = [(0, len(q) - 1)]
        while stack:
            lo, hi = stack.pop()
            if hi - lo < 2:
                continue
            a, b, r = q[lo], q[hi], q[lo + 1:hi] - q[lo]
            d = b - a
            if d[0] or d[1]:
                v = np.abs(d[0] * r[:, 1] - d[1] * r[:, 0])
                m = int(np.argmax(v))
                fv = np.float64(v[m])
                num, den = fv * fv, np.float64(d[0] * d[0] + d[1] * d[1])
            else:
                v = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
                m = int(np.argmax(v))
                num, den = np.float64(v[m]), np.float64(1.0)
            if num > e2 * den:
                keep[lo + 1 + m] = True
                stack.append((lo, lo + 1 + m))
                stack.append((lo + 1 + m, hi))
        out.append(p[keep[:length]])
    return np.concatenate(out).astype(np.int32) if out else np.zeros((0, 2), np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--eps", type=float, default=1.0)
    ap.add_argument("--host-points", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polylines_probe.json"))
    args = ap.parse_args()
    import torch
    import cvsteer_amd as cv
    import polyline_model
    res = {"device": torch.cuda.get_device_name(0), "eps": args.eps,
           "method": "wall clock around synchronising calls repeated over windows of >= %.1f s after one warm-up call, %d rounds, median; "
                     "the host walk once" % (args.window, args.rounds), "cases": []}

    def run(f, name, mask):
        rows, cols = mask.shape
        pts, table = f.contour_chains(mask)
        vtx, pol = f.chain_polylines(pts, table, args.eps)
        ms = [window(lambda: f.chain_polylines(pts, table, args.eps), args.window) for _ in range(args.rounds)]
        rec = {"rows": rows, "cols": cols, "input": name, "op": "chain_polylines", "chains": len(table), "points": len(pts),
               "vertices": len(vtx), "longest_chain": int(table[:, 1].max()) if len(table) else 0, "ms_rounds": ms, "ms": statistics.median(ms)}
        res["cases"].append(rec)
        print(rec, flush=True)
        hp, ht = pts.cpu().numpy(), table.cpu().numpy()
        lead = int(np.searchsorted(np.cumsum(ht[:, 1]), args.host_points, side="right")) or 1   # whole chains, at least one
        ht = ht[:lead]
        t0 = time.perf_counter()
        hv = host_polylines(hp, ht, args.eps)
        rec = {"rows": rows, "cols": cols, "input": name, "op": "host walk (numpy, this file)", "chains": len(ht),
               "points": int(ht[:, 1].sum()), "vertices": len(hv), "ms": 1e3 * (time.perf_counter() - t0)}
        res["cases"].append(rec)
        print(rec, flush=True)
        k = int(pol[:lead, 1].sum())
        assert np.array_equal(vtx[:k].cpu().numpy(), hv), "the device polylines differ from the host walk"
        few = int(np.searchsorted(np.cumsum(ht[:, 1]), 20000, side="right"))
        if few:
            mv, mt, _ = polyline_model.polylines(hp, ht[:few], args.eps)
            assert np.array_equal(vtx[:len(mv)].cpu().numpy(), mv) and np.array_equal(pol[:few].cpu().numpy(), mt), "... from the model"

    for rows, cols in ((4096, 4096), (1080, 1920)):
        g = torch.Generator(device=DEV).manual_seed(rows)
        img = torch.rand((rows, cols), device=DEV, generator=g)
        f = cv.SteerableFiltersG2(img)
        thin = f.nonmax(f.pipeline(img)[5:8])
        hi = max(float(t.max()) for t in thin)
        masks = f.contours(img, 0.05 * hi, 0.2 * hi)
        run(f, "chains of the thinned contours() edges mask of a noise image", masks[0])
    run(cv.SteerableFiltersG2(torch.rand((1024, 1024), device=DEV)), "chain of the 1-pixel serpentine", torch.from_numpy(serpentine()).to(DEV))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(res, fo, indent=1)


if __name__ == "__main__":
    main()
