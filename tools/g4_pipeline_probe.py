"""G4 caller pipeline (CVS_OPT_G4_EXTENSIONS = 1): rates of the fused path -- the pair launch and one per-pixel launch -- and of
the four-launch composition it replaces, in one process.  Prints ONE JSON line.

    python tools/g4_pipeline_probe.py [--window S] [--rounds R]

Timed with device events on the handles' stream, after warm-up, over windows of at least --window seconds:
  fused_state_4096      pipeline() on a 4096^2 image, all 8 outputs, state kept
  fused_nostate_4096    the same image, set_persist(False), three maps (edges, dark, bright) only
  batch_1080p_x32       pipeline_batch() of 32 x 1080p frames, three maps only, no state
  composed_4096         setup(FULL) + steer(None, full=True) + find(magnitude, phase) on the 4096^2 image, all 8 outputs --
                        alternated with fused_state_4096 round by round (the *_ab entries)
Every entry gives ms per call (per batch), Mpix/s, and GB/s against two byte counts, named:
  algorithmic  what the result needs: image in + kept state + outputs (with state 4 + 44 + 20 + 32 = 100 B/pix; three
               maps without state 4 + 12 = 16 B/pix)
  moved        what this design moves: with state 4 + 44 (pair launch) + 44 + 20 + 32 (per-pixel launch) = 144 B/pix; three
               maps without state 4 + 44 + 44 + 12 = 104 B/pix; the composition 212 B/pix
The per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--window 0.2)."""
import argparse
import json
import statistics
import sys
import os

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cvsteer_amd as cv  # noqa: E402

BYTES = {"state": {"algorithmic": 100, "moved": 144}, "three": {"algorithmic": 16, "moved": 104},
         "composed": {"algorithmic": 100, "moved": 212}}


def timed(fn, window):
    """ms per call of fn(), device events around a run of calls that lasts at least `window` seconds"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= window * 1e3:
            return ms / n
        n = max(2 * n, int(n * window * 1.2e3 / max(ms, 1e-3)) + 1)


def entry(ms, npix, counts):
    d = {"ms": round(ms, 4), "mpix_per_s": round(npix / ms / 1e3, 1)}
    for name, b in counts.items():
        d["gbps_" + name] = round(npix * b / ms / 1e6, 1)
        d["bytes_per_pix_" + name] = b
    d["hbm_fraction_moved"] = round(npix * counts["moved"] / ms / 1e6 / 8000.0, 3)   # of the 8 TB/s HBM peak
    return d


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="alternating composed / fused rounds")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("g4_pipeline_probe needs a HIP device")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(4096)
    n = 4096
    img = torch.rand((n, n), generator=g, device=dev) * 255
    npix = n * n
    res = {"probe": "g4_pipeline", "window_s": args.window}

    fused = cv.SteerableFiltersG4(None, 6, 0.5, extensions=True)
    outs8 = cv.alloc_planes(8, n, n, device=dev)
    composed = cv.SteerableFiltersG4(None, 6, 0.5, extensions=True)
    five = cv.alloc_planes(5, n, n, device=dev)
    feat = cv.alloc_planes(3, n, n, device=dev)

    def run_fused():
        fused.pipeline(img, out=outs8)

    def run_composed():
        composed.setup(img, cv.SETUP_FULL)
        gg, hh, e, m, p = composed.steer(None, full=True, out=five)
        composed.find(m, p)   # (find allocates its three maps per call, like the library's Python callers)

    # same values, or the comparison means nothing
    run_fused()
    run_composed()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(outs8[:5], five))
    ab_f, ab_c = [], []
    for _ in range(args.rounds):
        ab_c.append(timed(run_composed, args.window))
        ab_f.append(timed(run_fused, args.window))
    res["fused_state_4096"] = entry(statistics.median(ab_f), npix, BYTES["state"])
    res["composed_4096"] = entry(statistics.median(ab_c), npix, BYTES["composed"])
    res["ab_rounds_ms"] = {"fused": [round(v, 4) for v in ab_f], "composed": [round(v, 4) for v in ab_c]}
    res["composed_over_fused"] = round(statistics.median(ab_c) / statistics.median(ab_f), 3)
    res["composed_equals_fused"] = bool(same)

    stateless = cv.SteerableFiltersG4(None, 6, 0.5, extensions=True)
    stateless.set_persist(False)
    res["fused_nostate_4096"] = entry(timed(lambda: stateless.pipeline(img, out=[None] * 5 + feat), args.window), npix, BYTES["three"])
    del outs8, five, feat, fused, composed, stateless
    torch.cuda.empty_cache()

    nf, rows, cols = 32, 1080, 1920
    frames = torch.rand((nf, rows, cols), generator=g, device=dev) * 255
    out = torch.empty((nf, 3, rows, cols), dtype=torch.float32, device=dev)
    batch = cv.SteerableFiltersG4(None, 6, 0.5, extensions=True)
    batch.set_persist(False)
    res["batch_1080p_x32"] = entry(timed(lambda: batch.pipeline_batch(frames, out=out, outputs=(5, 6, 7)), args.window), nf * rows * cols,
                                   BYTES["three"])
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
