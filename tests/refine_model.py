"""numpy / Python models of the contour edgels (cvs_chain_refine, cvs_chain_measures) -- TEST INFRASTRUCTURE ONLY, written from the contract
in include/cvsteer_hip.h, not from the kernels.

refine_map is the contract on every pixel of a map at once, one numpy operation per operation of the contract, in float32 (each numpy
operation on float32 arrays rounds on its own, the division is correctly rounded) or, with dtype=float64, the same formulas in double.
(c, s) are arguments, so a test may pass the oracle's polar_to_cart (directions) or nudge them.  measures is plain Python: a loop over the
chains, exact sums (math.fsum) of the terms the contract names."""
import math

import numpy as np

import contour_model as CM

F32 = np.float32
CLOSED = 1
MEASURE_DTYPE = np.dtype([("axial", "<i4"), ("diagonal", "<i4"), ("other", "<i4"), ("peak_index", "<i4"), ("peak", "<f4"),
                          ("weakest", "<f4"), ("sum", "<f8"), ("length", "<f8")])

directions = CM.directions


def samples(m, c, s, dtype=F32):
    """(vb, vf, w, major_x) of the cvs_nonmax contract on every pixel, in `dtype`; neighbours outside the image read as 0"""
    m = np.ascontiguousarray(m, dtype=dtype)
    c, s = np.asarray(c, dtype=dtype), np.asarray(s, dtype=dtype)
    rows, cols = m.shape
    p = np.pad(m, 1)

    def at(dr, dc):
        return p[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols]

    with np.errstate(all="ignore"):
        ax, ay = np.abs(c), np.abs(s)
        major_x = ax >= ay
        w = np.where(major_x, ay / ax, ax / ay).astype(dtype)
        om = (dtype(1.0) - w).astype(dtype)
        cpos, spos = c >= 0, s >= 0          # forward column step +1 / forward row step -1
        f_row = {dc: np.where(spos, at(-1, dc), at(1, dc)) for dc in (-1, 0, 1)}
        b_row = {dc: np.where(spos, at(1, dc), at(-1, dc)) for dc in (-1, 0, 1)}
        diag_f = np.where(cpos, f_row[1], f_row[-1])
        diag_b = np.where(cpos, b_row[-1], b_row[1])
        side_f = np.where(major_x, np.where(cpos, at(0, 1), at(0, -1)), f_row[0])
        side_b = np.where(major_x, np.where(cpos, at(0, -1), at(0, 1)), b_row[0])
        vf = ((om * side_f).astype(dtype) + (w * diag_f).astype(dtype)).astype(dtype)
        vb = ((om * side_b).astype(dtype) + (w * diag_b).astype(dtype)).astype(dtype)
    return vb, vf, w, major_x


def refine_map(m, c, s, dtype=F32):
    """the contract of cvs_chain_refine on every pixel: a dict of planes -- t, xs, ys, strength, and what they came from (a, b, vb, vf, w,
    keep, m)"""
    m = np.ascontiguousarray(m, dtype=dtype)
    c, s = np.asarray(c, dtype=dtype), np.asarray(s, dtype=dtype)
    vb, vf, w, major_x = samples(m, c, s, dtype)
    rows, cols = m.shape
    y, x = np.mgrid[0:rows, 0:cols]
    with np.errstate(all="ignore"):
        a = (m - vb).astype(dtype)
        b = (m - vf).astype(dtype)
        keep = (a > 0) & (b >= 0)
        diff = (a - b).astype(dtype)
        t = np.where(keep, (dtype(0.5) * (diff / (a + b).astype(dtype)).astype(dtype)).astype(dtype), dtype(0.0)).astype(dtype)
        tw = np.where(keep, (t * w).astype(dtype), dtype(0.0)).astype(dtype)
        tx, ty = np.where(major_x, t, tw), np.where(major_x, tw, t)
        xs = (x.astype(dtype) + np.where(c >= 0, tx, -tx)).astype(dtype)
        ys = (y.astype(dtype) + np.where(s >= 0, -ty, ty)).astype(dtype)
        strength = np.where(keep, (m + (dtype(0.25) * (diff * t).astype(dtype)).astype(dtype)).astype(dtype), m).astype(dtype)
    return dict(t=t, xs=xs, ys=ys, strength=strength, a=a, b=b, vb=vb, vf=vf, w=w, keep=keep, m=m)


def gather(planes, points):
    """(xy (N, 2), strength (N,)) of a refine_map result at `points` ((x, y) pairs); a point outside the image gives NaN"""
    points = np.asarray(points, np.int64).reshape(-1, 2)
    rows, cols = planes["m"].shape
    dt = planes["xs"].dtype
    x, y = points[:, 0], points[:, 1]
    inside = (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
    xy = np.full((len(points), 2), np.nan, dt)
    st = np.full((len(points),), np.nan, dt)
    xy[inside, 0] = planes["xs"][y[inside], x[inside]]
    xy[inside, 1] = planes["ys"][y[inside], x[inside]]
    st[inside] = planes["strength"][y[inside], x[inside]]
    return xy, st


def refine(points, m, theta, dtype=F32):
    """cvs_chain_refine: (xy, strength) with (c, s) from the oracle's polar_to_cart"""
    c, s = directions(theta)
    return gather(refine_map(m, c, s, dtype), points)


def measures(points, chains, strength=None, xy=None, return_abs=False):
    """cvs_chain_measures on host arrays: a MEASURE_DTYPE array, sums exact (math.fsum) and rounded once.  return_abs: also the sums of the
    absolute terms of `sum` and `length`, per chain -- what a bound on the error of an order of additions is made of"""
    points = np.asarray(points, np.int64).reshape(-1, 2)
    out = np.zeros(len(chains), MEASURE_DTYPE)
    abs_sum, abs_len = np.zeros(len(chains)), np.zeros(len(chains))
    for k, (start, n, flags, _) in enumerate(np.asarray(chains).reshape(-1, 4).tolist()):
        rec = out[k]
        if start < 0 or n < 1 or start + n > len(points):
            rec["peak_index"] = -1
            continue
        steps = n - 1 + (1 if flags & CLOSED else 0)
        lens = []
        for i in range(steps):
            p, q = start + i, start + (i + 1) % n
            dx, dy = int(points[q, 0] - points[p, 0]), int(points[q, 1] - points[p, 1])
            kind = "axial" if abs(dx) + abs(dy) == 1 else "diagonal" if abs(dx) == 1 and abs(dy) == 1 else "other"
            rec[kind] += 1
            if xy is not None:
                dx, dy = float(xy[q][0]) - float(xy[p][0]), float(xy[q][1]) - float(xy[p][1])
            lens.append(math.sqrt(float(dx) * float(dx) + float(dy) * float(dy)))
        rec["length"] = math.fsum(lens) if all(math.isfinite(v) for v in lens) else float(np.sum(lens))
        abs_len[k] = rec["length"]
        rec["peak_index"], rec["peak"], rec["weakest"] = -1, -np.inf, np.inf
        if strength is not None:
            vals = [float(v) for v in np.asarray(strength)[start:start + n]]
            rec["sum"] = math.fsum(vals) if all(math.isfinite(v) for v in vals) else float(np.sum(vals))
            abs_sum[k] = math.fsum(abs(v) for v in vals if math.isfinite(v))
            real = [(v, i) for i, v in enumerate(vals) if not math.isnan(v)]
            if real:
                peak = max(v for v, _ in real)
                rec["peak"], rec["weakest"] = peak, min(v for v, _ in real)
                rec["peak_index"] = start + min(i for v, i in real if v == peak)
    return (out, abs_sum, abs_len) if return_abs else out


# ---- geometry: straight ridges through (size // 2 + 0.3, size // 2 + 0.1) ----
GEOMETRY_ANGLES = [22.5 * k for k in range(8)] + [10.0, 37.0, 71.0, 100.0, 133.0]


def ridge(size, deg, seed=0):
    """(image, theta, distance): exp(-d^2 / 4.5) + 0.002 noise around the line at `deg` degrees (x right, y down), theta analytic -- (cos
    theta, -sin theta) is the line's normal -- and distance(x, y), the signed distance of a position from the line, in float64"""
    a = np.deg2rad(deg)
    nx, ny = -np.sin(a), np.cos(a)

    def distance(x, y):
        return (np.asarray(x, np.float64) - size // 2 - 0.3) * nx + (np.asarray(y, np.float64) - size // 2 - 0.1) * ny

    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    d = distance(x, y)
    img = np.exp(-d * d / 4.5) + 0.002 * np.random.default_rng(seed).random((size, size))
    theta = np.full((size, size), np.arctan2(-ny, nx), F32)
    return img.astype(F32), theta, distance
