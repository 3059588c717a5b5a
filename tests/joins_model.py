"""Model of cvs_chain_joins (plain Python and numpy, no GPU): written from the contract in include/cvsteer_hip.h, not from the kernels.  It
imports nothing from the library.

All arithmetic is float64, one rounding per operation (neither Python nor numpy fuses anything), with explicit narrowing to float32 where
the contract stores a float.  The arm sums are built literally: term 1 first, then term 2 added to it, ... in ascending k.  The nodes are
a dict from the key (R, y, x) to the list of the ends there."""
import numpy as np

JOIN_DTYPE = np.dtype([("node", "<i4"), ("degree", "<i4"), ("next", "<i4"), ("partner", "<i4"), ("flags", "<i4"), ("n", "<i4"), ("cos", "<f4"),
                       ("sin", "<f4")])
MUTUAL, NONE, CROWDED, SHORT, DEGENERATE, NO_CHAIN = 1, 2, 4, 8, 16, 32
INELIGIBLE = NONE | CROWDED | SHORT | DEGENERATE | NO_CHAIN
CLOSED = 1
MAX_DEGREE = 8
QNAN_BITS = 0x7FC00000
_QNAN = np.uint32(QNAN_BITS).view(np.float32)


def _arm(X, j, sign, n):
    """the arm of `n` points from position j: (a.x, a.y, len)"""
    x0, y0 = X[j]
    sx = sy = None
    for k in range(1, n + 1):
        tx, ty = X[j + sign * k, 0] - x0, X[j + sign * k, 1] - y0
        sx, sy = (tx, ty) if k == 1 else (sx + tx, sy + ty)
    ax, ay = sx / np.float64(n), sy / np.float64(n)
    return ax, ay, np.sqrt(ax * ax + ay * ay)


def _pair(A, e, f):
    """(cos, sin) of the turn from arriving through end e to leaving through end f, as float32.  The cross product is formed once per
    pair, from the smaller end number to the larger, and the sine of the other direction is that sine with its sign bit flipped."""
    lo, hi = min(e, f), max(e, f)
    (ax, ay, la), (bx, by, lb) = A[lo], A[hi]
    den = la * lb
    dt = -(ax * bx + ay * by)
    cr = ay * bx - ax * by
    cs, sn = np.float32(dt / den), np.float32(cr / den)
    return cs, (sn if e < f else -sn)


def joins(points, chains, xy=None, radius=8, min_arm=None, min_cos=-1.0):
    """the table of cvs_chain_joins, 2 records per chain, for any table a DEVICE call accepts"""
    min_arm = min(3, radius) if min_arm is None else min_arm
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    chains = np.asarray(chains, np.int64).reshape(-1, 4)
    n_points, m = len(pts), len(chains)
    X = pts.astype(np.float64) if xy is None else np.asarray(xy, np.float32).reshape(-1, 2).astype(np.float64)
    out = np.zeros(2 * m, JOIN_DTYPE)
    out["node"] = out["next"] = out["partner"] = -1
    out["cos"] = out["sin"] = _QNAN
    out["flags"] = NONE
    arms, nodes = {}, {}
    with np.errstate(all="ignore"):
        for c, (S, L, F, R) in enumerate(chains.tolist()):
            if not (S >= 0 and L >= 1 and S + L <= n_points):
                out["flags"][2 * c:2 * c + 2] = NONE | NO_CHAIN
                continue
            if (F & CLOSED) or L < 2:
                continue
            n = min(radius, L - 1)
            for e, j, sign in ((2 * c, S, +1), (2 * c + 1, S + L - 1, -1)):
                a = _arm(X, j, sign, n)
                arms[e] = a
                out["n"][e] = n
                out["flags"][e] = (SHORT if n < min_arm else 0) | (0 if (a[2] > 0 and np.isfinite(a[2])) else DEGENERATE)
                nodes.setdefault((R, int(pts[j, 1]), int(pts[j, 0])), []).append(e)
        for ends in nodes.values():                                            # (ascending: the chains were visited in order)
            d = len(ends)
            for k, e in enumerate(ends):
                out["node"][e], out["degree"][e] = ends[0], d
                if d > MAX_DEGREE:
                    out["flags"][e] |= CROWDED
                else:
                    out["next"][e] = ends[(k + 1) % d]
        elig = (out["flags"] & INELIGIBLE) == 0
        for ends in nodes.values():
            for e in ends:
                if not elig[e]:
                    continue
                best = None
                for f in ends:
                    if f == e or not elig[f]:
                        continue
                    cs, sn = _pair(arms, e, f)
                    if best is None or cs > best[1]:
                        best = (f, cs, sn)
                if best is not None:
                    out["partner"][e], out["cos"][e], out["sin"][e] = best
        partner = out["partner"].copy()
        for e in np.nonzero(partner >= 0)[0]:
            if partner[partner[e]] == e and out["cos"][e] >= np.float32(min_cos):
                out["flags"][e] |= MUTUAL
    return out


def host_table_wrong(n_points, chains):
    """is a HOST call with this table refused: the starts are the running sum of the lengths from 0 to n_points, every length >= 1"""
    at = 0
    for s, ln in np.asarray(chains, np.int64).reshape(-1, 4)[:, :2].tolist():
        if ln < 1 or s != at:
            return True
        at += ln
    return at != n_points


def walk_mutual(table, start):
    """the ends visited by following MUTUAL joins from the free end `start`: into the chain at `start`, out of its other end, through the
    mutual join there into the partner's chain, ... ; stops at an end without a mutual join"""
    seen, e = [], int(start)
    while True:
        other = e ^ 1                                                          # the chain's other end
        if e in seen or other in seen:
            return seen + [e]                                                  # (a repeat: the caller asserts there is none)
        seen += [e, other]
        if not table["flags"][other] & MUTUAL:
            return seen
        e = int(table["partner"][other])


def same_records(a, b):
    """two tables, byte for byte; a difference is reported by field and position"""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, a.shape, b.dtype, b.shape)
    for name in a.dtype.names:
        x, y = np.ascontiguousarray(a[name]).view(np.uint32), np.ascontiguousarray(b[name]).view(np.uint32)
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, "%s differs at %d position(s), the first %s: 0x%08X, not 0x%08X" % (name, len(bad), bad[:8].tolist(), int(x[bad[0]]), int(y[bad[0]]))
    return a.tobytes() == b.tobytes()
