"""Model of cvs_chain_bridges (plain Python and numpy, no GPU): written from the contract in include/cvsteer_hip.h, not from the kernels.  It
imports nothing from the library.

Sequential throughout: the arm of every end (float64, one rounding per operation, term 1 first), the crowding of the cells from a dict,
then for every candidate ALL other candidates of its plane -- no cells, no lists: that every partner in range lies in the nine cells
around an end is the contract's theorem, not the model's method -- and the bridges one point at a time in Python integers."""
import numpy as np

BRIDGE_DTYPE = np.dtype([("partner", "<i4"), ("flags", "<i4"), ("n", "<i4"), ("steps", "<i4"), ("bridge", "<i4"), ("start", "<i4"),
                         ("cos", "<f4"), ("cos_partner", "<f4")])
MUTUAL, NONE, JUNCTION, SHORT, DEGENERATE, NO_CHAIN, CROWDED = 1, 2, 4, 8, 16, 32, 64
NOT_CANDIDATE = NONE | JUNCTION | SHORT | DEGENERATE | NO_CHAIN | CROWDED
CLOSED, HEAD_JUNCTION, TAIL_JUNCTION = 1, 2, 4
MAX_CELL = 32
QNAN_BITS = 0x7FC00000
_QNAN = np.uint32(QNAN_BITS).view(np.float32)


def _arm(X, j, sign, n):
    """the arm of `n` points from position j: (a.x, a.y, len) -- the arm of cvs_chain_joins"""
    x0, y0 = X[j]
    sx = sy = None
    for k in range(1, n + 1):
        tx, ty = X[j + sign * k, 0] - x0, X[j + sign * k, 1] - y0
        sx, sy = (tx, ty) if k == 1 else (sx + tx, sy + ty)
    ax, ay = sx / np.float64(n), sy / np.float64(n)
    return ax, ay, np.sqrt(ax * ax + ay * ay)


def line(x0, y0, x1, y1):
    """the digital line of a bridge from (x0, y0) to (x1, y1), steps + 1 points, in Python integers"""
    dx, dy = x1 - x0, y1 - y0
    steps = max(abs(dx), abs(dy))
    return [(x0 + (2 * j * dx + steps) // (2 * steps), y0 + (2 * j * dy + steps) // (2 * steps)) for j in range(steps + 1)]


def bridges(points, chains, xy=None, radius=8, min_arm=3, max_gap=8, min_cos=0.8, cap_points=None, cap_chains=None):
    """what cvs_chain_bridges writes, for any tables a DEVICE call accepts: (table, out_points, out_chains, out_xy, counts).  table: 2
    records per chain (BRIDGE_DTYPE); out_points (P, 2) int32, out_chains (K, 4) int32 and out_xy ((P, 2) float32, None without xy) hold
    what a call with these capacities WRITES -- the copies and the prefix of the bridges that fits (cap None: everything) --; counts =
    (n_bridges, n_out_chains, n_out_points), the full totals whatever the capacities."""
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    ch = np.asarray(chains, np.int64).reshape(-1, 4).tolist()
    n_points, m = len(pts), len(ch)
    fxy = None if xy is None else np.ascontiguousarray(np.asarray(xy, np.float32).reshape(-1, 2))
    X = pts.astype(np.float64) if fxy is None else fxy.astype(np.float64)
    fmin = np.float32(min_cos)
    out = np.zeros(2 * m, BRIDGE_DTYPE)
    out["partner"] = out["bridge"] = out["start"] = -1
    out["cos"] = out["cos_partner"] = _QNAN
    out["flags"] = NONE
    arms, pos = {}, {}
    with np.errstate(all="ignore"):
        for c, (S, L, F, R) in enumerate(ch):
            if not (S >= 0 and L >= 1 and S + L <= n_points):
                out["flags"][2 * c:2 * c + 2] = NONE | NO_CHAIN
                continue
            if (F & CLOSED) or L < 2:
                continue
            n = min(radius, L - 1)
            for e, j, sign, bit in ((2 * c, S, +1, HEAD_JUNCTION), (2 * c + 1, S + L - 1, -1, TAIL_JUNCTION)):
                a = _arm(X, j, sign, n)
                arms[e], pos[e] = a, j
                out["n"][e] = n
                out["flags"][e] = ((JUNCTION if F & bit else 0) | (SHORT if n < min_arm else 0)
                                   | (0 if (a[2] > 0 and np.isfinite(a[2])) else DEGENERATE))
        # crowding: the candidates before it, counted per cell (floor division: Python's //)
        cell = {e: (ch[e >> 1][3], int(pts[j, 1]) // max_gap, int(pts[j, 0]) // max_gap) for e, j in pos.items()}
        count = {}
        for e in sorted(pos):
            if not out["flags"][e] & NOT_CANDIDATE:
                count[cell[e]] = count.get(cell[e], 0) + 1
        crowded = {k for k, v in count.items() if v > MAX_CELL}
        for e, (R, cy, cx) in cell.items():
            if any((R, cy + dy, cx + dx) in crowded for dy in (-1, 0, 1) for dx in (-1, 0, 1)):
                out["flags"][e] |= CROWDED
        cand = np.array([e for e in sorted(pos) if not out["flags"][e] & NOT_CANDIDATE], np.int64)
        at = np.array([pos[e] for e in cand], np.int64)
        px, py = pts[at, 0], pts[at, 1]                                              # int64: the INTEGER points
        pr = np.array([ch[e >> 1][3] for e in cand], np.int64)
        CX, CY = X[at, 0], X[at, 1]                                                  # float64: the coordinates
        AX, AY, AL = (np.array([arms[e][k] for e in cand], np.float64) for k in range(3))
        for i, e in enumerate(cand.tolist()):
            # every other candidate of the plane that is in range, all at once: each line below is one rounded operation per element
            near = np.maximum(np.abs(px - px[i]), np.abs(py - py[i]))
            sel = np.nonzero((pr == pr[i]) & (near >= 2) & (near <= max_gap))[0]
            if len(sel) == 0:
                continue
            f = cand[sel]
            up = f > e                                                               # e is lo
            dx, dy = np.where(up, px[sel] - px[i], px[i] - px[sel]), np.where(up, py[sel] - py[i], py[i] - py[sel])
            d2 = dx * dx + dy * dy
            Dx, Dy = np.where(up, CX[sel] - CX[i], CX[i] - CX[sel]), np.where(up, CY[sel] - CY[i], CY[i] - CY[sel])
            dlen = np.sqrt(Dx * Dx + Dy * Dy)
            lax, lay, ll = np.where(up, AX[i], AX[sel]), np.where(up, AY[i], AY[sel]), np.where(up, AL[i], AL[sel])
            hax, hay, hl = np.where(up, AX[sel], AX[i]), np.where(up, AY[sel], AY[i]), np.where(up, AL[sel], AL[i])
            cos_lo = (-(lax * Dx + lay * Dy) / (ll * dlen)).astype(np.float32)
            cos_hi = ((hax * Dx + hay * Dy) / (hl * dlen)).astype(np.float32)
            ok = np.isfinite(dlen) & (dlen > 0) & (cos_lo >= fmin) & (cos_hi >= fmin)
            if not ok.any():
                continue
            k = np.nonzero(ok)[0]
            k = k[np.lexsort((f[k], d2[k]))[0]]                                      # the smallest (d2, f)
            out["partner"][e], out["steps"][e] = f[k], near[sel][k]
            out["cos"][e], out["cos_partner"][e] = (cos_lo[k], cos_hi[k]) if up[k] else (cos_hi[k], cos_lo[k])
    partner = out["partner"].copy()
    for e in np.nonzero(partner >= 0)[0]:
        if partner[partner[e]] == e:
            out["flags"][e] |= MUTUAL

    # the bridges: MUTUAL pairs by ascending lo
    cap_points = (1 << 62) if cap_points is None else cap_points
    cap_chains = (1 << 62) if cap_chains is None else cap_chains
    assert cap_points >= n_points and cap_chains >= m
    o_pts = [tuple(p) for p in pts.tolist()]
    o_xy = None if fxy is None else [fxy[i].copy() for i in range(n_points)]
    o_ch = [list(c) for c in ch]
    for e in np.nonzero(out["flags"] & MUTUAL)[0].tolist():
        o_ch[e >> 1][2] |= TAIL_JUNCTION if e & 1 else HEAD_JUNCTION
    k, at = 0, n_points
    for lo in range(2 * m):
        hi = int(partner[lo])
        if not (out["flags"][lo] & MUTUAL) or hi < lo:
            continue
        steps = int(out["steps"][lo])
        for e in (lo, hi):
            out["bridge"][e], out["start"][e] = k, np.int64(at).astype(np.int32)
        if m + k < cap_chains and at + steps < cap_points:
            assert len(o_ch) == m + k and len(o_pts) == at, "the bridges that are written are a prefix"
            (x0, y0), (x1, y1) = pts[pos[lo]].tolist(), pts[pos[hi]].tolist()
            o_pts += line(x0, y0, x1, y1)
            o_ch.append([at, steps + 1, HEAD_JUNCTION | TAIL_JUNCTION, ch[lo >> 1][3]])
            if o_xy is not None:
                c0, c1 = X[pos[lo]], X[pos[hi]]
                mid = [(c0 + (np.float64(j) / np.float64(steps)) * (c1 - c0)).astype(np.float32) for j in range(1, steps)]
                o_xy += [fxy[pos[lo]].copy()] + mid + [fxy[pos[hi]].copy()]
        k, at = k + 1, at + steps + 1
    counts = (k, m + k, at)
    return (out, np.asarray(o_pts, np.int64).astype(np.int32).reshape(-1, 2), np.asarray(o_ch, np.int64).astype(np.int32).reshape(-1, 4),
            None if o_xy is None else np.asarray(o_xy, np.float32).reshape(-1, 2), counts)


def same_bytes(name, got, want):
    """two arrays byte for byte, structured ones field by field first so that a failure names the field"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.dtype, want.shape)
    for f in got.dtype.names or ():
        x, y = np.ascontiguousarray(got[f]).view(np.uint32), np.ascontiguousarray(want[f]).view(np.uint32)
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, "%s.%s differs at %d position(s), the first %s: 0x%08X, not 0x%08X" % (
            name, f, len(bad), bad[:8].tolist(), int(x[bad[0]]), int(y[bad[0]]))
    if got.tobytes() != want.tobytes():
        a, b = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
        bad = np.nonzero(a != b)[0]
        raise AssertionError("%s differs at %d byte(s), the first at element %s" % (name, len(bad), (bad[:8] // max(got.itemsize, 1)).tolist()))
    return True
