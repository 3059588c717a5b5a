"""Python model of the contour polylines (cvs_chain_polylines) -- TEST ONLY, written from the contract in include/cvsteer_hip.h, not from the
kernels: the split rule segment by segment with an explicit stack (the kept set does not depend on the order of the visits), Python ints for
every value, numpy.float64 for the one floating-point test."""
import numpy as np

CLOSED = 1


def value(a, b, q):
    """v(i) of the split rule: |cross| for a != b, the squared distance from a otherwise (Python ints: exact)"""
    ax, ay = a
    bx, by = b
    qx, qy = q
    if a != b:
        return abs((bx - ax) * (qy - ay) - (by - ay) * (qx - ax))
    return (qx - ax) ** 2 + (qy - ay) ** 2


def splits(v, a, b, eps):
    """num > e2 * den in IEEE double, one rounding per operation; eps as the float32 the call takes"""
    e = np.float64(np.float32(eps))
    e2 = e * e
    if a != b:
        dx, dy = b[0] - a[0], b[1] - a[1]
        fv = np.float64(v)
        num, den = fv * fv, np.float64(dx * dx + dy * dy)
    else:
        num, den = np.float64(v), np.float64(1.0)
    with np.errstate(over="ignore"):
        return bool(num > e2 * den)


def virtual_list(pts, closed):
    q = [(int(x), int(y)) for x, y in pts]
    return q + [q[0]] if closed else q


def split_point(q, lo, hi):
    """(m, v(m)): the smallest interior index with the largest value"""
    best, m = -1, -1
    for i in range(lo + 1, hi):
        v = value(q[lo], q[hi], q[i])
        if v > best:
            best, m = v, i
    return m, best


def kept(pts, closed, eps):
    """sorted indices into pts of the points of one chain that are kept"""
    n_real = len(pts)
    if n_real <= 2:
        return list(range(n_real))
    q = virtual_list(pts, closed)
    n = len(q)
    keep = {0, n - 1}
    stack = [(0, n - 1)]
    while stack:
        lo, hi = stack.pop()
        if hi - lo < 2:
            continue
        m, v = split_point(q, lo, hi)
        if splits(v, q[lo], q[hi], eps):
            keep.add(m)
            stack.append((lo, m))
            stack.append((m, hi))
    return sorted(i for i in keep if i < n_real)   # the repeated point of a closed chain is virtual


def polylines(points, chains, eps):
    """cvs_chain_polylines: (vertices (V, 2) int32, table (M, 4) int32 of (start, length, flags, 0), index (V,) int32)"""
    points = np.asarray(points, np.int32).reshape(-1, 2)
    chains = np.asarray(chains, np.int32).reshape(-1, 4)
    index, table = [], []
    for start, length, flags, _ in chains.tolist():
        assert start >= 0 and length >= 1 and start + length <= len(points)
        k = kept(points[start:start + length].tolist(), bool(flags & CLOSED), eps)
        table.append((len(index), len(k), flags, 0))
        index.extend(start + i for i in k)
    index = np.array(index, np.int32).reshape(-1)
    return points[index].reshape(-1, 2), np.array(table, np.int32).reshape(-1, 4), index
