"""Orientation peaks against the composition they replace: one MI355X process, 4096^2, the same handle for both,
alternated in timed windows of >= 1 s after warm-up, device events around each window.

  python tools/peaks_probe.py [--size 4096] [--window 1.0] [--rounds 3] [--out profiles/peaks_probe.json]

The composition: steer_bank(theta_0 .. theta_(K-1), outputs=(0, 1)) into a preallocated block, then rules 2-9 of the contract
(include/cvsteer_hip.h) as torch expressions on those planes -- the energies, the range, the candidate mask, torch.topk for the M
strongest (which orders ties as it likes: the cheaper stand-in for the contract's order), the gathered neighbours and the parabola.
Bytes per pixel of the call: reads 4 nb, writes 8 M + 1; of the bank alone: reads 4 nb, writes 8 K."""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cvsteer_amd as cv  # noqa: E402
from cvsteer_amd import _lib as L  # noqa: E402

CASES = [("G2", 16, 2), ("G4", 16, 2)]
THRESHOLDS = (0.0, 0.25, 1e-3)   # the defaults of orientation_peaks


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


def torch_rules(g, h, M, me, mr, mc):
    """rules 2-9 on the bank's planes g, h [K, H, W] -> angles[M], energies[M], count (uint8)"""
    K = g.shape[0]
    e = g * g + h * h
    emax, emin = e.amax(0), e.amin(0)
    pixel = torch.isfinite(e).all(0) & ((emax - emin) > mc * emax)
    prev, nxt = e.roll(1, 0), e.roll(-1, 0)
    cand = (e > prev) & (e >= nxt) & (e > me) & (e >= mr * emax) & pixel
    key = torch.where(cand, e, torch.full_like(e, -math.inf))
    c, k = key.topk(M, dim=0)
    valid = torch.isfinite(c)
    p, n = prev.gather(0, k), nxt.gather(0, k)
    num = p - n
    den = (p - 2.0 * c) + n
    d = torch.where(den < 0, (0.5 * num) / den, torch.zeros_like(den)).clamp(-0.5, 0.5)
    ang = (k.to(torch.float32) + d) * np.float32(math.pi / K)
    ang = torch.where(ang < 0, ang + np.float32(math.pi), ang)
    ang = torch.where(ang >= np.float32(math.pi), ang - np.float32(math.pi), ang)
    en = c - (0.25 * num) * d
    return (torch.where(valid, ang, torch.full_like(ang, -1.0)), torch.where(valid, en, torch.zeros_like(en)),
            cand.sum(0).clamp(max=M).to(torch.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peaks_probe.json"))
    args = ap.parse_args()
    n = args.size
    img = torch.from_numpy(np.random.default_rng(7).random((n, n), dtype=np.float32)).cuda()
    handles = {"G2": cv.SteerableFiltersG2(img), "G4": cv.SteerableFiltersG4(img)}
    rows = []
    for kind, K, M in CASES:
        f = handles[kind]
        th = np.array([np.float32(np.float64(k) * np.pi / K) for k in range(K)], np.float32)
        outs = f.orientation_peaks(K, M, *THRESHOLDS)
        bank = f.steer_bank(th)
        # both sides call the library straight from prebuilt descriptors: no per-call Python marshalling in the timed windows
        cfg = L.PeaksCfg(ctypes.sizeof(L.PeaksCfg), K, M, *THRESHOLDS)
        pa, pe, pc = cv.api._planes(list(outs[0])), cv.api._planes(list(outs[1])), cv.api._plane(outs[2])
        bplanes = (L.Plane * (5 * K))()
        for t in range(K):
            for o in (0, 1):
                bplanes[5 * t + o] = cv.api._plane(bank[o][t])
        thp = th.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

        def peaks():
            f._bind_stream(img)
            rc = L.lib().cvs_orientation_peaks(f._h, ctypes.byref(cfg), pa, pe, ctypes.byref(pc))
            assert rc == 0, rc

        def bank_only():
            f._bind_stream(img)
            rc = L.lib().cvs_steer_bank(f._h, thp, K, bplanes)
            assert rc == 0, rc

        def composition():
            bank_only()
            return torch_rules(bank[0], bank[1], M, *THRESHOLDS)

        # the two agree wherever no tie or rounding decides (the composition contracts nothing either, but topk orders ties freely)
        ref = composition()
        torch.cuda.synchronize()
        agree = float((ref[2] == outs[2]).float().mean())
        tp, tc, tb = [], [], []
        for _ in range(args.rounds):
            tp.append(window(peaks, args.window))
            tc.append(window(composition, args.window))
            tb.append(window(bank_only, args.window))
        nb = 7 if kind == "G2" else 11
        ms_p, ms_c, ms_b = float(np.median(tp)), float(np.median(tc)), float(np.median(tb))
        row = {"bank": kind, "K": K, "M": M, "thresholds": list(THRESHOLDS), "bytes_per_pix": 4 * nb + 8 * M + 1,
               "bank_bytes_per_pix": 4 * nb + 8 * K, "peaks_ms": round(ms_p, 4), "composition_ms": round(ms_c, 4),
               "bank_alone_ms": round(ms_b, 4), "speedup": round(ms_c / ms_p, 2), "count_agreement": round(agree, 6),
               "peaks_ms_all": [round(x, 4) for x in tp], "composition_ms_all": [round(x, 4) for x in tc],
               "bank_alone_ms_all": [round(x, 4) for x in tb]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del outs, bank, ref
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"size": n, "window_s": args.window, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
