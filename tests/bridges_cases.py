"""The inputs of the bridge tests (test_bridges_cpu.py, test_gpu_bridges.py): masks and hand-made tables, built once.  No GPU, nothing
of the library: chains come from chains_model."""
import functools

import numpy as np

import chains_model as CM

F32 = np.float32
SHAPE = (33, 65)
DASH, GAP = 6, 3
# (radius, min_arm, max_gap, min_cos): radius 1, 8 and 64 (min_arm 3, held to the radius), max_gap 2, 5 and 32, min_cos -1 and 0.8
CONFIGS = tuple((radius, min(3, radius), max_gap, min_cos) for radius in (1, 8, 64) for max_gap in (2, 5, 32) for min_cos in (-1.0, 0.8))


def _frozen(*arrays):
    out = tuple(None if a is None else np.ascontiguousarray(a) for a in arrays)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def dashed_pixels(kind):
    """the pixels of a dashed line, dashes of 6 and gaps of 3, and its number of dashes: `horizontal` (row 16, from x = 2, 7 dashes),
    `vertical` (column 32, from y = 1, 3 dashes), `diagonal` (from (5, 3) down to the right, 3 dashes)"""
    dashes = {"horizontal": 7, "vertical": 3, "diagonal": 3}[kind]
    ks = [k for k in range(dashes * (DASH + GAP) - GAP)]
    at = {"horizontal": lambda k: (2 + k, 16), "vertical": lambda k: (32, 1 + k), "diagonal": lambda k: (5 + k, 3 + k)}[kind]
    return [at(k) for k in ks if k % (DASH + GAP) < DASH], [at(k) for k in ks], dashes


def dashed_mask(kind):
    mask = np.zeros(SHAPE, F32)
    for x, y in dashed_pixels(kind)[0]:
        mask[y, x] = 1
    return mask


def jitter(pts):
    """the points plus a fixed sub-pixel jitter"""
    return (np.asarray(pts) + np.random.default_rng(len(pts) + 1).uniform(-0.4, 0.4, np.asarray(pts).shape)).astype(F32)


def random_mask(density):
    return (np.random.default_rng(int(1000 * density) + 3).random((64, 64)) < density).astype(F32)


def crowd_table():
    """40 two-pixel chains inside the cell x, y = 8 .. 15 (80 free ends: crowded at max_gap 8), 6 in its neighbour x = 16 .. 23 (CROWDED by
    their neighbour), and two facing pairs of three-pixel dashes far away, which bridge"""
    rng = np.random.default_rng(40)
    pts = []
    for lo, count in ((8, 40), (16, 6)):
        for _ in range(count):
            x, y = int(rng.integers(lo, lo + 7)), int(rng.integers(8, 16))
            pts += [(x, y), (x + 1, y)]
    tab = [[2 * c, 2, 0, 0] for c in range(46)]
    for y in (40, 50):
        tab += [[len(pts), 3, 0, 0], [len(pts) + 3, 3, 0, 0]]
        pts += [(40, y), (41, y), (42, y), (46, y), (47, y), (48, y)]
    return np.int32(pts), np.int32(tab)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (points, chains, jittered xy), read-only"""
    out = {}
    for kind in ("horizontal", "vertical", "diagonal"):
        out[kind] = CM.chains(dashed_mask(kind))
    for density in (0.05, 0.2):
        out["random %.2f" % density] = CM.chains(random_mask(density))
    out["crowd"] = crowd_table()
    return {name: _frozen(np.asarray(p, np.int32), np.asarray(c, np.int32), jitter(p)) for name, (p, c) in out.items()}


def two_planes():
    """the horizontal dashed line in two planes of a batch table: every free end coincides in (y, x) with one of the other plane"""
    pts, chains, xy = cases()["horizontal"]
    second = np.array(chains)
    second[:, 0] += len(pts)
    second[:, 3] = 1
    return _frozen(np.concatenate([pts, pts]), np.concatenate([chains, second]), np.concatenate([xy, xy]))


def shifted(name, dx, dy):
    """a case moved by (dx, dy): coordinates may turn negative"""
    pts, chains, xy = cases()[name]
    return _frozen(pts + np.int32([dx, dy]), chains, (xy + F32([dx, dy])).astype(F32))
