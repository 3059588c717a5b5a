"""numpy / Python model of the contour segments (cvs_polyline_segments) -- TEST INFRASTRUCTURE ONLY, written from the contract in
include/cvsteer_hip.h, not from the kernels.

spans is the span rule, vertex by vertex, with what the contract says a DEVICE table that breaks it yields (the record without a span).
terms are the six terms of every point of a span as numpy float64 operations (each rounds on its own); exact_sums adds them as
fractions.Fraction -- exactly -- and rounds once, and returns the sums of the absolute terms a bound on any order of additions is made of.
derive is the derived sequence of the contract operation by operation on numpy.float64 scalars (IEEE double, division and sqrt correctly
rounded, no contraction), dmax the second pass, vectorised.  segments puts them together into records."""
from fractions import Fraction

import numpy as np

CLOSED = 1
WRAPS, DEGENERATE = 1, 2
SUMS = ("w", "sx", "sy", "sxx", "sxy", "syy")
DERIVED = ("cx", "cy", "ux", "uy", "t0", "t1", "rms", "dmax")
SEGMENT_DTYPE = np.dtype([("first", "<i4"), ("count", "<i4"), ("chain", "<i4"), ("flags", "<i4")] + [(n, "<f8") for n in SUMS + DERIVED])
F64 = np.float64


def spans(chains, polylines, index, n_points=None):
    """one (first, count, chain, flags, positions) per vertex: positions = the span's positions in `points` (an int64 array), None where no
    span starts at the vertex.  n_points: the length of the point list the chain entries are checked against (None: the largest end)"""
    chains = np.asarray(chains, np.int64).reshape(-1, 4)
    polylines = np.asarray(polylines, np.int64).reshape(-1, 4)
    index = np.asarray(index, np.int64).reshape(-1)
    if n_points is None:
        n_points = int((chains[:, 0] + chains[:, 1]).max()) if len(chains) else 0
    out = []
    for k in range(len(index)):
        c = 0
        for cand in range(len(polylines)):                                  # the largest c with polylines[c].start <= k, never outside the table
            if polylines[cand, 0] <= k:
                c = cand
        # (a sorted table makes this the binary search's answer; on an unsorted one the search is only required to stay inside the table)
        S, L, F = (int(v) for v in chains[c, :3])
        vs, vl = int(polylines[c, 0]), int(polylines[c, 1])
        i0 = int(index[k])
        none = (i0, 0, c, 0, None)
        if S < 0 or L < 1 or S + L > n_points or vs < 0 or not (vs <= k < vs + vl) or not (S <= i0 < S + L):
            out.append(none)
        elif k + 1 < vs + vl:
            i1 = int(index[k + 1]) if k + 1 < len(index) else -1
            if not (S <= i1 < S + L) or i0 >= i1:
                out.append(none)
            else:
                out.append((i0, i1 - i0 + 1, c, 0, np.arange(i0, i1 + 1, dtype=np.int64)))
        elif F & CLOSED:
            iv = int(index[vs])
            if not (S <= iv < S + L) or iv > i0:
                out.append(none)
            else:
                pos = np.concatenate([np.arange(i0, S + L, dtype=np.int64), np.arange(S, iv + 1, dtype=np.int64)])
                out.append((i0, len(pos), c, WRAPS, pos))
        else:
            out.append(none)
    return out


def offsets(points, xy, first, pos):
    """(dx, dy) of the points at `pos` from the span's first pixel, float64: exact for |coordinates| < 2^28"""
    x0, y0 = F64(points[first][0]), F64(points[first][1])
    src = points if xy is None else xy
    with np.errstate(all="ignore"):
        dx = np.asarray(src)[pos, 0].astype(F64) - x0
        dy = np.asarray(src)[pos, 1].astype(F64) - y0
    return dx, dy


def weights(strength, pos):
    if strength is None:
        return np.ones(len(pos), F64)
    s = np.asarray(strength, np.float32)[pos]
    with np.errstate(invalid="ignore"):
        return np.where(s > 0, s.astype(F64), F64(0.0))                     # (false for NaN)


def terms(points, xy, strength, first, pos):
    """the six terms of every point of a span, (6, count) float64, each operation rounded on its own"""
    dx, dy = offsets(points, xy, first, pos)
    w = weights(strength, pos)
    with np.errstate(all="ignore"):
        wx, wy = w * dx, w * dy
        return np.stack([w, wx, wy, wx * dx, wx * dy, wy * dy])


def exact_sums(points, chains, polylines, index, xy=None, strength=None, n_points=None):
    """per vertex (sums, abs_sums): six floats each -- the exact sums of the terms rounded once, and the sums of the |terms|; (None, None)
    where no span starts.  A span with a term that is not finite gets the plain IEEE sums instead (NaN or an infinity either way)"""
    points = np.asarray(points, np.int64).reshape(-1, 2)
    out = []
    for first, count, _, _, pos in spans(chains, polylines, index, len(points) if n_points is None else n_points):
        if pos is None:
            out.append((None, None))
            continue
        t = terms(points, xy, strength, first, pos)
        if np.isfinite(t).all():
            sums = [float(sum((Fraction(float(v)) for v in row), Fraction(0))) for row in t]
            mags = [float(sum((Fraction(abs(float(v))) for v in row), Fraction(0))) for row in t]
        else:
            with np.errstate(all="ignore"):
                sums, mags = [float(row.sum()) for row in t], [float(np.abs(row).sum()) for row in t]
        out.append((sums, mags))
    return out


def derive(sums, first_d, last_d, origin):
    """the derived sequence of the contract on six sums: a dict of mx, my, cx, cy, ux, uy, t0, t1, rms and `degenerate`.  first_d / last_d:
    (dx, dy) of the span's first and last point; origin: (x0, y0).  numpy.float64 scalars: one IEEE operation per Python operation"""
    w, sx, sy, sxx, sxy, syy = (F64(v) for v in sums)
    fx, fy = F64(first_d[0]), F64(first_d[1])
    lx, ly = F64(last_d[0]), F64(last_d[1])
    x0, y0 = F64(origin[0]), F64(origin[1])
    zero, half, nan = F64(0.0), F64(0.5), F64(np.nan)
    with np.errstate(all="ignore"):
        mx = sx / w
        my = sy / w
        a = sxx - sx * mx
        b = sxy - sx * my
        c = syy - sy * my
        d = a - c
        e = b + b
        r = np.sqrt(d * d + e * e)
        vx, vy = (d + r, e) if d >= zero else (e, r - d)
        hh = np.sqrt(vx * vx + vy * vy)
        ux = vx / hh
        uy = vy / hh
        qx, qy = lx - fx, ly - fy
        s = ux * qx + uy * qy
        if s < zero or (s == zero and (ux < zero or (ux == zero and uy < zero))):
            ux, uy = -ux, -uy
        cx = x0 + mx
        cy = y0 + my
        t0 = ux * (fx - mx) + uy * (fy - my)
        t1 = ux * (lx - mx) + uy * (ly - my)
        lmin = half * ((a + c) - r)
        rms = np.sqrt((lmin if lmin > zero else zero) / w)
        degenerate = bool(not (w > zero) or not (hh > zero) or np.isinf(hh))
    if degenerate:
        ux = uy = t0 = t1 = rms = nan
    return dict(mx=mx, my=my, cx=cx, cy=cy, ux=ux, uy=uy, t0=t0, t1=t1, rms=rms, degenerate=degenerate)


def dmax(dx, dy, line):
    """the second pass: the largest |ux (dy - my) - uy (dx - mx)| over all points of the span (NaN for a degenerate line)"""
    if line["degenerate"]:
        return F64(np.nan)
    with np.errstate(all="ignore"):
        v = np.abs(line["ux"] * (dy - line["my"]) - line["uy"] * (dx - line["mx"]))
    v = v[~np.isnan(v)]
    return F64(v.max()) if len(v) else F64(0.0)


def finish(rec, points, xy, pos):
    """fill the eight derived fields and the DEGENERATE flag of a record from ITS OWN six sums (first, count, flags and sums are set)"""
    dx, dy = offsets(points, xy, int(rec["first"]), pos)
    line = derive([rec[n] for n in SUMS], (dx[0], dy[0]), (dx[-1], dy[-1]), points[int(rec["first"])])
    for n in DERIVED[:-1]:
        rec[n] = line[n]
    rec["dmax"] = dmax(dx, dy, line)
    if line["degenerate"]:
        rec["flags"] |= DEGENERATE


def segments(points, chains, polylines, index, xy=None, strength=None, return_abs=False, n_points=None):
    """cvs_polyline_segments on host arrays: a SEGMENT_DTYPE array, the sums exact and rounded once, the line derived from them.
    return_abs: also the (V, 6) sums of the absolute terms"""
    points = np.asarray(points, np.int64).reshape(-1, 2)
    n_points = len(points) if n_points is None else n_points
    sp = spans(chains, polylines, index, n_points)
    ex = exact_sums(points, chains, polylines, index, xy, strength, n_points)
    out = np.zeros(len(sp), SEGMENT_DTYPE)
    mags = np.zeros((len(sp), 6))
    for k, ((first, count, chain, flags, pos), (sums, mag)) in enumerate(zip(sp, ex)):
        rec = out[k]
        rec["first"], rec["count"], rec["chain"], rec["flags"] = first, count, chain, flags
        if pos is None:
            continue
        for n, v in zip(SUMS, sums):
            rec[n] = v
        mags[k] = mag
        finish(rec, points, xy, pos)
    return (out, mags) if return_abs else out


def end_points(seg):
    """(N, 4) float64: (cx + t0 ux, cy + t0 uy, cx + t1 ux, cy + t1 uy)"""
    return np.stack([seg["cx"] + seg["t0"] * seg["ux"], seg["cy"] + seg["t0"] * seg["uy"],
                     seg["cx"] + seg["t1"] * seg["ux"], seg["cy"] + seg["t1"] * seg["uy"]], axis=1).reshape(-1, 4)
