"""cvsteer-run for MI355X: the reference's batch driver (example/steer.cpp:59-173) over the HIP engine.

    python -m cvsteer_amd.run --input <image | list.txt> --output <dir> [--gain G] [--g4] [--contours LOW,HIGH[,MIN_AREA[,MIN_PEAK]]]
    python -m torch.distributed.run --nproc-per-node 8 -m cvsteer_amd.run --input list.txt --output out

Per image, exactly the reference's per-file body (steer.cpp:69-124): gray f32 (unscaled 0..255) ->
SteerableFiltersG2(gray, 4, 0.67) -> steer at the dominant orientation -> findEdges / findDarkLines /
findBrightLines on the magnitude -> 8-bit via normalize(0,255,MINMAX) or convertTo(gain) ->
<base>_edges.png, <base>_lines_dark.png, <base>_lines_bright.png.  --g4 runs the same sequence on the
G4/H4 bank instead (SteerableFiltersG4(gray, 6, 0.5) with extensions on: steered at the G4 dominant
orientation -- an extension, the reference's G4 class has no orientation or find*).  All arithmetic, including the
8-bit conversion, runs on the GPU; only file decoding/encoding is host work (Pillow / numpy, since
OpenCV's imgcodecs are not available).

The reference parallelises over files with cv::parallel_for_ (steer.cpp:169); here the file list is
sharded over the ranks of a torch.distributed job (one process per GPU, contiguous blocks) and each
rank walks its block -- no collective is needed on the data path.

Differences from the reference, on purpose: `--gain` is honoured (the reference passes `--verbose`
as the gain, steer.cpp:167-168); single-channel inputs work (the reference leaves `gray` empty for
them, steer.cpp:79-82); unreadable files are reported, not silently skipped.
"""
import argparse
import os
import sys

import numpy as np

from .batch import shard_range


def read_gray(path):
    """image file -> 2-D array (uint8 or float32), the caller-side imread + BGR2GRAY of steer.cpp:73-82"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path)
    else:
        from PIL import Image
        a = np.asarray(Image.open(path).convert("L"))
    if a.ndim == 3:  # H x W x C -> luma, ITU-R 601 like cv::COLOR_BGR2GRAY (channels assumed RGB)
        a = a[..., :3].astype(np.float32) @ np.array([0.299, 0.587, 0.114], np.float32)
    if a.ndim != 2:
        raise ValueError("%s: expected a 2-D (gray) or 3-D (colour) image" % path)
    return a


def write_u8(path, u8):
    if path.lower().endswith(".npy"):
        np.save(path, u8)
    else:
        from PIL import Image
        Image.fromarray(u8).save(path)


def input_list(arg):
    """steer.cpp:156-165: a .txt file (or a name without extension) is a list of files, else one image"""
    if arg.endswith(".txt") or "." not in os.path.basename(arg):
        with open(arg) as f:
            return [ln.strip() for ln in f if ln.strip()]
    return [arg]


def process_file(engine, path, outdir, gain, ext=".png"):
    import torch
    gray = read_gray(path)
    dev = torch.device("cuda", engine.device)
    img = torch.from_numpy(np.ascontiguousarray(gray))
    if img.dtype != torch.uint8:
        img = img.to(torch.float32)
    img = img.to(dev)  # 8-bit images cross PCIe as bytes and are widened by the engine (CVS_DEPTH_U8)
    # one launch; only the three feature maps leave it, as bytes (set_persist(False): no state planes): convertTo(gain) in the
    # kernel's epilogue, or normalize(NORM_MINMAX) with min / max reduced in the launch and one quantise launch behind it
    engine.set_u8_gain(gain if gain > 0 else 0.0)
    feat = [torch.empty(tuple(img.shape), dtype=torch.uint8, device=dev) for _ in range(3)]
    outs = engine.pipeline(img, out=[None] * 5 + feat)
    base = os.path.splitext(os.path.basename(path))[0]
    written = []
    for u8, suffix in zip(outs[5:], ("_edges", "_lines_dark", "_lines_bright")):
        if outdir:
            dst = os.path.join(outdir, base + suffix + ext)
            write_u8(dst, u8.cpu().numpy())
            written.append(dst)
    return written


def contours_arg(text):
    """--contours LOW,HIGH[,MIN_AREA[,MIN_PEAK]] -> (low, high, min_area, min_peak); argparse turns the errors into exit status 2"""
    parts = text.split(",")
    if not 2 <= len(parts) <= 4:
        raise argparse.ArgumentTypeError("expected LOW,HIGH[,MIN_AREA[,MIN_PEAK]], not %r" % text)
    try:
        low, high = float(parts[0]), float(parts[1])
        min_area = int(parts[2]) if len(parts) > 2 else 0
        min_peak = float(parts[3]) if len(parts) > 3 else 0.0
    except ValueError:
        raise argparse.ArgumentTypeError("expected numbers (MIN_AREA an integer), not %r" % text)
    if not low <= high:   # (NaN fails the test as well)
        raise argparse.ArgumentTypeError("LOW <= HIGH, neither NaN")
    if min_area < 0 or min_peak != min_peak:
        raise argparse.ArgumentTypeError("MIN_AREA >= 0, MIN_PEAK not NaN")
    return low, high, min_area, min_peak


def process_contours(engine, paths, outdir, contours, ext=".png", chunk=32):
    """--contours: thin, linked contours instead of the 8-bit maps.  Files of equal size and depth go through contours_batch in chunks of
    up to `chunk` frames (one upload, one chain of launches, one download); the three 0 / 255 masks get the names of the maps.
    -> (files written, [(path, error)])"""
    import torch
    dev = torch.device("cuda", engine.device)
    low, high, min_area, min_peak = contours
    groups, failed, written = {}, [], []
    for path in paths:
        try:
            gray = np.ascontiguousarray(read_gray(path))
            if gray.dtype != np.uint8:
                gray = gray.astype(np.float32)
            groups.setdefault((gray.shape, gray.dtype.str), []).append((path, gray))
        except Exception as exc:
            failed.append((path, exc))
    for items in groups.values():
        for i in range(0, len(items), chunk):
            part = items[i:i + chunk]
            try:
                frames = torch.from_numpy(np.stack([g for _, g in part])).to(dev)
                masks = engine.contours_batch(frames, low, high, min_area, min_peak).cpu().numpy()
                for (path, _), m in zip(part, masks):
                    base = os.path.splitext(os.path.basename(path))[0]
                    for u8, suffix in zip(m, ("_edges", "_lines_dark", "_lines_bright")):
                        if outdir:
                            dst = os.path.join(outdir, base + suffix + ext)
                            write_u8(dst, u8)
                            written.append(dst)
            except Exception as exc:
                failed.extend((path, exc) for path, _ in part)
    return written, failed


def main(argv=None):
    ap = argparse.ArgumentParser(prog="cvsteer-run", description=__doc__.split("\n")[0])
    ap.add_argument("--input", required=True, help="image file, or a .txt list of image files")
    ap.add_argument("--output", default="", help="output directory")
    ap.add_argument("--gain", type=float, default=0.0, help="gain for the 8-bit output (0 = min-max normalise)")
    ap.add_argument("--ext", default=".png", help="output file extension (.png, .pgm, .npy ...)")
    ap.add_argument("--g4", action="store_true", help="the G4/H4 bank (width 6, spacing 0.5, extensions on) instead of G2/H2")
    ap.add_argument("--contours", type=contours_arg, default=None, metavar="LOW,HIGH[,MIN_AREA[,MIN_PEAK]]",
                    help="write thin, linked contours (0 / 255 masks under the same names) instead of the 8-bit maps: hysteresis "
                         "thresholds on the thinned maps, then components of fewer than MIN_AREA pixels or with a peak below MIN_PEAK "
                         "are dropped; files of equal size are processed in batches")
    ap.add_argument("--verbose", action="store_true")
    args = ap.parse_args(argv)

    import torch
    from . import SteerableFiltersG2, SteerableFiltersG4

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("cvsteer-run needs a HIP device (there is no CPU fallback)")
    files = input_list(args.input)
    lo, hi = shard_range(len(files), world, rank)
    if args.output:
        os.makedirs(args.output, exist_ok=True)
    if args.g4:
        engine = SteerableFiltersG4(None, 6, 0.5, device=local_rank, extensions=True)
    else:
        engine = SteerableFiltersG2(None, 4, 0.67, device=local_rank)
    if args.contours is not None:   # thinning reads every frame's theta plane: the state stays on
        written, errors = process_contours(engine, files[lo:hi], args.output, args.contours, args.ext)
        if args.verbose:
            print("[rank %d] %d files -> %d masks" % (rank, hi - lo, len(written)), flush=True)
        for path, exc in errors:
            print("[rank %d] %s: %s" % (rank, path, exc), file=sys.stderr, flush=True)
        return 1 if errors else 0
    engine.set_persist(False)  # the driver never revisits an image's basis planes
    failed = 0
    for path in files[lo:hi]:
        try:
            written = process_file(engine, path, args.output, args.gain, args.ext)
            if args.verbose:
                print("[rank %d] %s -> %s" % (rank, path, ", ".join(written) or "(not written)"), flush=True)
        except Exception as exc:  # the reference `continue`s silently on unreadable files
            failed += 1
            print("[rank %d] %s: %s" % (rank, path, exc), file=sys.stderr, flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
