"""Contour chains and edgels on the batch axis on one MI355X: one contour_chains_batch call against the loop of
contour_chains calls it replaces, and one chain_refine_batch call against the loop of select_frame + chain_refine, in one process.

Input: the thinned, linked masks of contours_batch on 32 noise frames of 1920 x 1080 -- all 96 planes, [96, H, W] uint8 on the device -- and
the un-thinned maps of the same frames for the refinement (theta: the state the batch left in the object).  The two sides of a comparison
alternate: a warm-up call of each, then windows of >= 1 s of repeated calls with the stream synchronised around them, three rounds, medians.

  python tools/chains_batch_probe.py [--frames 32] [--rows 1080] [--cols 1920] [--window 1.0] [--rounds 3] [--out profiles/chains_batch_probe.json]

The table prints ms per pass over all planes, and loop / batch."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def window(fn, seconds):
    """fn repeated over >= `seconds` of wall time between two synchronisations -> ms per call"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e3 * dt / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chains_batch_probe.json"))
    args = ap.parse_args()
    import torch
    import cvsteer_amd as cv

    torch.manual_seed(7)
    frames = torch.rand((args.frames, args.rows, args.cols), device=DEV) * 255
    f = cv.SteerableFiltersG2(frames[0])
    maps = f.pipeline_batch(frames, outputs=[5, 6, 7])
    hi = float(f.nonmax_batch(maps).max())
    masks = f.contours_batch(frames, 0.05 * hi, 0.2 * hi)
    n = 3 * args.frames
    flat = masks.reshape(n, args.rows, args.cols)
    torch.cuda.synchronize()

    def chains_batch():
        return f.contour_chains_batch(flat)

    def chains_loop():
        return [f.contour_chains(flat[z]) for z in range(n)]

    points, chains, ranges = chains_batch()
    each = chains_loop()
    assert sum(len(p) for p, _ in each) == len(points) and sum(len(t) for _, t in each) == len(chains)
    assert torch.equal(torch.cat([p for p, _ in each]), points)

    def refine_batch():
        return f.chain_refine_batch(points, ranges, maps)

    def refine_loop():
        out = []
        for z in range(n):
            f.select_frame(z // 3)
            out.append(f.chain_refine(each[z][0], maps[z // 3, z % 3]))
        return out

    xy, _ = refine_batch()
    assert torch.equal(torch.cat([a for a, _ in refine_loop()]).view(torch.int32), xy.view(torch.int32))
    torch.cuda.synchronize()

    sides = {"contour_chains_batch": chains_batch, "contour_chains_loop": chains_loop, "chain_refine_batch": refine_batch,
             "chain_refine_loop": refine_loop}
    times = {k: [] for k in sides}
    for _ in range(args.rounds):
        for name, fn in sides.items():   # batch, loop, batch, loop: the two sides of a comparison alternate
            times[name].append(window(fn, args.window))
    med = {k: statistics.median(v) for k, v in times.items()}
    result = {
        "device": torch.cuda.get_device_name(0), "frames": args.frames, "rows": args.rows, "cols": args.cols, "planes": n,
        "chains": int(len(chains)), "points": int(len(points)), "window_s": args.window, "rounds": args.rounds,
        "ms_per_pass": {k: round(v, 4) for k, v in med.items()}, "ms_rounds": {k: [round(x, 4) for x in v] for k, v in times.items()},
        "loop_over_batch": {"contour_chains": round(med["contour_chains_loop"] / med["contour_chains_batch"], 3),
                            "chain_refine": round(med["chain_refine_loop"] / med["chain_refine_batch"], 3)},
    }
    print("%d planes of %d x %d: %d chains, %d points" % (n, args.rows, args.cols, len(chains), len(points)))
    for a, b in (("contour_chains_batch", "contour_chains_loop"), ("chain_refine_batch", "chain_refine_loop")):
        print("%-22s %9.3f ms   %-20s %9.3f ms   loop / batch %.2f" % (a, med[a], b, med[b], med[b] / med[a]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
