"""Steering bank against K separate scalar steers: one MI355X process, 4096^2, the same handle and the
same output planes for both, alternated in timed windows of >= 1 s after warm-up, device events around each window.

  python tools/steer_bank_probe.py [--size 4096] [--window 1.0] [--rounds 3] [--out profiles/steer_bank_probe.json]
  python tools/steer_bank_probe.py --trace-only   # a few bank calls of each case and nothing else (for rocprofv3 --kernel-trace)

Bytes per pixel and call: reads 4 nb (+ 12 with e), writes 4 x kinds x K; the fraction is of 8 TB/s."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cvsteer_amd as cv  # noqa: E402
from cvsteer_amd import _lib as L  # noqa: E402

ROOF = 8.0e12
CASES = [("G2", k, (0, 1)) for k in (1, 2, 4, 8, 16, 32)] + [("G2", 8, (0, 1, 2, 3, 4)), ("G2", 8, (2,)), ("G4", 8, (0, 1))]
NAMES = ("g", "h", "e", "magnitude", "phase")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steer_bank_probe.json"))
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    n = args.size
    img = torch.from_numpy(np.random.default_rng(7).random((n, n), dtype=np.float32)).cuda()
    handles = {"G2": cv.SteerableFiltersG2(img), "G4": cv.SteerableFiltersG4(img)}
    rows = []
    for kind, k, kinds in CASES:
        f = handles[kind]
        th = np.linspace(0, np.pi, k, endpoint=False).astype(np.float32)
        outs = f.steer_bank(th, outputs=kinds)
        if args.trace_only:
            for _ in range(3):
                f.steer_bank(th, outputs=kinds, out=outs)
            torch.cuda.synchronize()
            print("traced", kind, k, kinds, flush=True)
            continue
        # the scalar calls write the very same planes, one angle at a time; cvs_steer_scalar always writes g and h, so where the
        # bank is not asked for them they go to scratch planes of the same size
        spare = [torch.empty(n, n, device="cuda") for _ in range(2)]
        planes = [[cv.api._plane(outs[kinds.index(o)][t]) if o in kinds else (cv.api._plane(spare[o]) if o < 2 else None)
                   for o in range(5)] for t in range(k)]
        ptrs = [[ctypes.byref(p) if p is not None else None for p in ps] for ps in planes]

        def scalar_calls():
            f._bind_stream(img)
            for t in range(k):
                rc = L.lib().cvs_steer_scalar(f._h, float(th[t]), *ptrs[t])
                assert rc == 0, rc

        # both sides call the library straight from prebuilt descriptors: no per-call Python marshalling in the timed windows
        bplanes = (L.Plane * (5 * k))()
        for t in range(k):
            for o in kinds:
                bplanes[5 * t + o] = cv.api._plane(outs[kinds.index(o)][t])
        thp = th.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

        def bank():
            f._bind_stream(img)
            rc = L.lib().cvs_steer_bank(f._h, thp, k, bplanes)
            assert rc == 0, rc

        tb, ts = [], []
        for _ in range(args.rounds):
            tb.append(window(bank, args.window))
            ts.append(window(scalar_calls, args.window))
        nb = 7 if kind == "G2" else 11
        bpp = 4 * nb + (12 if 2 in kinds else 0) + 4 * len(kinds) * k
        ms_b, ms_s = float(np.median(tb)), float(np.median(ts))
        row = {"bank": kind, "K": k, "kinds": [NAMES[o] for o in kinds], "bytes_per_pix": bpp,
               "bank_ms": round(ms_b, 4), "separate_ms": round(ms_s, 4), "speedup": round(ms_s / ms_b, 2),
               "bank_roof_frac": round(bpp * n * n / (ms_b * 1e-3) / ROOF, 3),
               "bank_ms_all": [round(x, 4) for x in tb], "separate_ms_all": [round(x, 4) for x in ts]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del outs, spare, planes, ptrs
    if not args.trace_only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"size": n, "window_s": args.window, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
                       "roof_Bps": ROOF, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
