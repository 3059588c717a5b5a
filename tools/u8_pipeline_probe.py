"""8-bit pipeline outputs: the three-maps launch with bytes out (fused) against the f32 launch followed by the min / max and quantise
passes (composed: cvs_pipeline_batch, then cvs_normalize_u8_batch / cvs_convert_u8_batch), alternated round by round in one process.
Prints ONE JSON line.

    python tools/u8_pipeline_probe.py [--window S] [--rounds R]

Timed with device events on the handles' stream, after warm-up, over windows of at least --window seconds, in gain (3.0) and in
normalise mode (gain 0):
  batch_1080p_x32   32 x 1080p uint8 frames in, edges / dark / bright as bytes out
  single_4096       one 4096^2 f32 image
  g4_batch_1080p_x8 the G4/H4 bank (extensions on): 8 x 1080p uint8 frames, one pair launch per frame + one per-pixel launch
Every entry gives ms per call, Gpix/s, and the bytes per pixel each route moves (image in + maps out + the passes behind it).
The kernel list comes from a separate `rocprofv3 --kernel-trace --stats` run of this script (--window 0.2 --rounds 1)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cvsteer_amd as cv  # noqa: E402
from cvsteer_amd import _lib as L  # noqa: E402


def timed(fn, window):
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


def case(frames, gain, g4=False):
    """(fused(), composed(), check()) for an [n, H, W] block of frames"""
    n, rows, cols = (int(v) for v in frames.shape)
    f = cv.SteerableFiltersG4(None, 6, 0.5, extensions=True) if g4 else cv.SteerableFiltersG2(None, 4, 0.67)
    f.set_persist(False)
    f.set_u8_gain(gain)
    out8 = torch.empty((n, 3, rows, cols), dtype=torch.uint8, device="cuda")
    out32 = torch.empty((n, 3, rows, cols), dtype=torch.float32, device="cuda")
    ref8 = torch.empty_like(out8)
    src = (L.Plane * (3 * n))(*[L.Plane(out32.data_ptr() + i * rows * cols * 4, rows, cols, cols * 4, L.MEM_DEVICE) for i in range(3 * n)])
    dst = (C.c_void_p * (3 * n))(*[ref8.data_ptr() + i * rows * cols for i in range(3 * n)])

    def fused():
        f.pipeline_batch(frames, out=out8, outputs=[5, 6, 7])

    def composed():
        f.pipeline_batch(frames, out=out32, outputs=[5, 6, 7])
        rc = (L.lib().cvs_convert_u8_batch(f._h, src, 3 * n, gain, 0.0, dst, cols, L.MEM_DEVICE) if gain > 0
              else L.lib().cvs_normalize_u8_batch(f._h, src, 3 * n, dst, cols, L.MEM_DEVICE))
        assert rc == 0, rc

    def check():
        fused()
        mode = f.launch_info()["u8_out"]
        composed()
        torch.cuda.synchronize()
        return mode, bool(torch.equal(out8, ref8))
    return fused, composed, check


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(5)
    forms = {
        "batch_1080p_x32": torch.randint(0, 256, (32, 1080, 1920), dtype=torch.uint8, device="cuda", generator=g),
        "single_4096": torch.rand((1, 4096, 4096), device="cuda", generator=g),
        "g4_batch_1080p_x8": torch.randint(0, 256, (8, 1080, 1920), dtype=torch.uint8, device="cuda", generator=g),
    }
    res = {}
    for name, frames in forms.items():
        n, rows, cols = (int(v) for v in frames.shape)
        in_b = frames.element_size()
        for mode, gain in (("gain", 3.0), ("normalise", 0.0)):
            fused, composed, check = case(frames, gain, g4=name.startswith("g4"))
            u8_out, equal = check()
            tf, tc = [], []
            for _ in range(args.rounds):
                tf.append(timed(fused, args.window))
                tc.append(timed(composed, args.window))
            px = n * rows * cols
            basis = 88 if name.startswith("g4") else 0               # G4: 11 basis planes written by the pair launch and read back
            bf = basis + in_b + (3 if gain > 0 else 12 + 12 + 3)      # fused: bytes out; normalise: f32 scratch out + back in + bytes
            bc = basis + in_b + 12 + (12 + 3 if gain > 0 else 12 + 12 + 3)  # composed: f32 maps out, then (min/max +) quantise passes
            key = "%s_%s" % (name, mode)
            res[key] = {"u8_out": u8_out, "equal": equal,
                        "fused_ms": round(statistics.median(tf), 4), "composed_ms": round(statistics.median(tc), 4),
                        "fused_gpix_s": round(px / statistics.median(tf) / 1e6, 3), "composed_gpix_s": round(px / statistics.median(tc) / 1e6, 3),
                        "fused_b_per_pix": bf, "composed_b_per_pix": bc,
                        "fused_all_ms": [round(v, 4) for v in tf], "composed_all_ms": [round(v, 4) for v in tc]}
    print(json.dumps({"probe": "u8_pipeline", "device": torch.cuda.get_device_name(0), "window_s": args.window, "results": res}))


if __name__ == "__main__":
    main()
