"""Model of cvs_chain_turns (numpy, no GPU): written from the contract in include/cvsteer_hip.h, not from the kernels.

All arithmetic is numpy float64, one rounding per operation (numpy fuses nothing), with explicit narrowing to float32 where the contract
stores a float.  The arm sums are built literally: term 1 first, then term 2 added to it, ... in ascending k.  The search for a point's
chain is the contract's binary search, written out, so that it is defined for any table."""
import numpy as np

TURN_DTYPE = np.dtype([("chain", "<i4"), ("flags", "<i4"), ("nb", "<i4"), ("nf", "<i4"), ("sin", "<f4"), ("cos", "<f4"), ("lb", "<f4"),
                       ("lf", "<f4")])
SUMMARY_DTYPE = np.dtype([("corners", "<i4"), ("eligible", "<i4"), ("sharpest", "<i4"), ("min_cos", "<f4")])
CORNER, END, DEGENERATE, SHORT, NO_CHAIN = 1, 2, 4, 8, 16
INELIGIBLE = END | DEGENERATE | SHORT | NO_CHAIN
CLOSED = 1
QNAN_BITS = 0x7FC00000
COS45 = float(np.float32(np.cos(np.pi / 4)))


def find_chain(starts, i):
    """the binary search of the contract for every position of `i`: lo = 0, hi = m - 1; mid = lo + (hi - lo + 1) / 2; starts[mid] <= i
    moves lo to mid, else hi to mid - 1.  The largest c with starts[c] <= i where the starts ascend."""
    starts = np.asarray(starts, np.int64)
    i = np.asarray(i, np.int64)
    lo, hi = np.zeros(len(i), np.int64), np.full(len(i), len(starts) - 1, np.int64)
    while (lo < hi).any():
        act = lo < hi
        mid = lo + (hi - lo + 1) // 2
        go = starts[np.clip(mid, 0, len(starts) - 1)] <= i
        lo = np.where(act & go, mid, lo)
        hi = np.where(act & ~go, mid - 1, hi)
    return lo


def _arm(X, ok, i, S, Ln, j, count, radius, sign):
    """sum of the terms X[j + sign k] - X[j], k = 1 .. count, in ascending k, starting from term 1"""
    acc = np.zeros((len(i), 2), np.float64)
    for k in range(1, radius + 1):
        sel = ok & (count >= k)
        if not sel.any():
            break
        jj = (j + sign * k)[sel]
        ln = Ln[sel]
        jj = np.where(jj < 0, jj + ln, jj)
        jj = np.where(jj >= ln, jj - ln, jj)
        term = X[S[sel] + jj] - X[i[sel]]
        acc[sel] = term if k == 1 else acc[sel] + term
    return acc


def turns(points, chains, xy=None, radius=5, min_arm=None, nms=None, max_cos=COS45, summary=False):
    """the table of cvs_chain_turns (and the summary with summary=True), for any table a DEVICE call accepts"""
    min_arm = radius if min_arm is None else min_arm
    nms = radius if nms is None else nms
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    chains = np.asarray(chains, np.int64).reshape(-1, 4)
    n, m = len(pts), len(chains)
    out = np.zeros(n, TURN_DTYPE)
    sums = np.zeros(m, SUMMARY_DTYPE)
    sums["sharpest"], sums["min_cos"] = -1, np.inf
    if n == 0:
        return (out, sums) if summary else out
    X = pts.astype(np.float64) if xy is None else np.asarray(xy, np.float32).reshape(-1, 2).astype(np.float64)
    i = np.arange(n, dtype=np.int64)
    c = find_chain(chains[:, 0], i)
    S, Ln, F = chains[c, 0], chains[c, 1], chains[c, 2]
    ok = (S >= 0) & (Ln >= 1) & (S + Ln <= n) & (i >= S) & (i < S + Ln)
    j = i - S
    closed = (F & CLOSED) != 0
    half = np.minimum(radius, (Ln - 1) // 2)
    nb = np.where(ok, np.where(closed, half, np.minimum(radius, j)), 0)
    nf = np.where(ok, np.where(closed, half, np.minimum(radius, Ln - 1 - j)), 0)
    with np.errstate(all="ignore"):
        sb = _arm(X, ok, i, S, Ln, j, nb, radius, -1)
        sf = _arm(X, ok, i, S, Ln, j, nf, radius, +1)
        ab = np.where((nb > 0)[:, None], sb / np.maximum(nb, 1)[:, None].astype(np.float64), 0.0)
        af = np.where((nf > 0)[:, None], sf / np.maximum(nf, 1)[:, None].astype(np.float64), 0.0)
        la = np.where(nb > 0, np.sqrt(ab[:, 0] * ab[:, 0] + ab[:, 1] * ab[:, 1]), 0.0)
        lf = np.where(nf > 0, np.sqrt(af[:, 0] * af[:, 0] + af[:, 1] * af[:, 1]), 0.0)
        dinx, diny = -ab[:, 0], -ab[:, 1]
        cr = dinx * af[:, 1] - diny * af[:, 0]
        dt = dinx * af[:, 0] + diny * af[:, 1]
        den = la * lf
        end = ok & ((nb == 0) | (nf == 0))
        deg = ok & ~end & (~(den > 0) | ~np.isfinite(den))
        good = ok & ~end & ~deg
        sn = np.where(good, cr / np.where(good, den, 1.0), np.nan).astype(np.float32)
        cs = np.where(good, dt / np.where(good, den, 1.0), np.nan).astype(np.float32)
        lb32, lf32 = la.astype(np.float32), lf.astype(np.float32)
    sn_bits, cs_bits = sn.view(np.uint32).copy(), cs.view(np.uint32).copy()
    sn_bits[~good], cs_bits[~good] = QNAN_BITS, QNAN_BITS
    flags = np.where(ok, 0, NO_CHAIN)
    flags |= np.where(end, END, 0) | np.where(deg, DEGENERATE, 0) | np.where(ok & ((nb < min_arm) | (nf < min_arm)), SHORT, 0)
    out["chain"], out["nb"], out["nf"] = np.where(ok, c, -1), nb, nf
    out["sin"], out["cos"] = sn_bits.view(np.float32), cs_bits.view(np.float32)
    for name, v in (("lb", lb32), ("lf", lf32)):
        bits = np.where(ok, v, 0).astype(np.float32).view(np.uint32).copy()
        bits[np.isnan(v) & ok] = QNAN_BITS                                     # every NaN the call stores is this one
        out[name] = bits.view(np.float32)

    # corners: the plateau rule on the stored floats
    elig = (flags & INELIGIBLE) == 0
    cos = out["cos"]
    with np.errstate(invalid="ignore"):
        keep = elig & (cos <= np.float32(max_cos))
    reach = np.where(closed, np.minimum(nms, (Ln - 1) // 2), nms)
    for k in range(1, nms + 1):
        act = keep & (reach >= k)
        if not act.any():
            break
        for sign in (-1, +1):
            jj = j + sign * k
            inside = (jj >= 0) & (jj < Ln)
            has = act & (inside | closed)
            jj = np.where(jj < 0, jj + Ln, jj)
            jj = np.where(jj >= Ln, jj - Ln, jj)
            q = np.where(has, S + jj, 0)
            other = cos[q]
            with np.errstate(invalid="ignore"):
                wins = (cos < other) if sign < 0 else (cos <= other)
            keep &= ~(has & elig[q] & ~wins)
    flags |= np.where(keep, CORNER, 0)
    out["flags"] = flags
    if not summary:
        return out
    for cc in range(m):
        s, ln = int(chains[cc, 0]), int(chains[cc, 1])
        if s < 0 or ln < 1 or s + ln > n:
            continue
        pos = np.arange(s, s + ln)
        pos = pos[out["chain"][pos] == cc]
        fl = out["flags"][pos]
        el = pos[(fl & INELIGIBLE) == 0]
        sums["corners"][cc], sums["eligible"][cc] = int((fl & CORNER != 0).sum()), len(el)
        if len(el):
            best = el[np.argmin(out["cos"][el])]        # argmin: the first of equal minima
            sums["sharpest"][cc], sums["min_cos"][cc] = best, out["cos"][best]
    return out, sums


def host_table_wrong(n_points, chains):
    """is a HOST call with this table refused: the starts are the running sum of the lengths from 0 to n_points, every length >= 1"""
    at = 0
    for s, ln in np.asarray(chains, np.int64).reshape(-1, 4)[:, :2].tolist():
        if ln < 1 or s != at:
            return True
        at += ln
    return at != n_points


def pack(lists, closed):
    """(points, chains) of ordered point lists, chain after chain"""
    points = np.concatenate([np.asarray(p, np.int32).reshape(-1, 2) for p in lists]).astype(np.int32)
    chains, at = [], 0
    for p, cl in zip(lists, closed):
        chains.append((at, len(p), CLOSED if cl else 0, 0))
        at += len(p)
    return points, np.int32(chains).reshape(-1, 4)


def corner_ridge(size, deg_in, deg_out, seed=0):
    """(image, theta, vertex): a ridge that arrives at the vertex (size // 2 + 0.3, size // 2 + 0.1) along the direction deg_in and leaves
    it along deg_out (degrees, x right, y down) -- two rays from the vertex, exp(-d^2 / 4.5) + 0.002 noise of the distance d from the
    nearer ray, theta analytic as in refine_model.ridge: (cos theta, -sin theta) is the normal of the nearer ray"""
    vx, vy = size // 2 + 0.3, size // 2 + 0.1
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    best, theta = None, None
    for deg in (deg_in + 180.0, deg_out):                        # the two rays, both pointing away from the vertex
        a = np.deg2rad(deg)
        ux, uy = np.cos(a), np.sin(a)
        t = np.maximum((x - vx) * ux + (y - vy) * uy, 0.0)
        d = np.hypot(x - vx - t * ux, y - vy - t * uy)
        th = np.full((size, size), np.arctan2(-ux, -uy))         # normal (-uy, ux) = (cos th, -sin th)
        if best is None:
            best, theta = d, th
        else:
            theta = np.where(d < best, th, theta)
            best = np.minimum(d, best)
    img = np.exp(-best * best / 4.5) + 0.002 * np.random.default_rng(seed).random((size, size))
    return img.astype(np.float32), theta.astype(np.float32), (vx, vy)


def ridge_case(deg_in, deg_out, size=48):
    """(image, theta, vertex, mask) of corner_ridge: the mask is its thinned ridge by contour_model, a border of 6 pixels cleared"""
    import contour_model as NM
    img, theta, vertex = corner_ridge(size, deg_in, deg_out)
    c, s = NM.directions(theta)
    sel = NM.nonmax_parts(img, c, s)[0] > 0.5
    sel[:6], sel[-6:], sel[:, :6], sel[:, -6:] = False, False, False, False
    return img, theta, vertex, sel.astype(np.float32)


def same_records(a, b):
    """two tables, byte for byte; a difference is reported by field and position"""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, a.shape, b.dtype, b.shape)
    for name in a.dtype.names:
        x, y = np.ascontiguousarray(a[name]).view(np.uint32), np.ascontiguousarray(b[name]).view(np.uint32)
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, "%s differs at %d position(s), the first %s: 0x%08X, not 0x%08X" % (name, len(bad), bad[:8].tolist(), int(x[bad[0]]), int(y[bad[0]]))
    return a.tobytes() == b.tobytes()
