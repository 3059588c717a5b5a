"""numpy / Python model of the contour chains (cvs_contour_chains) -- TEST ONLY, written from the contract in include/cvsteer_hip.h, not from
the kernels: links vectorised, then a plain walk from every node along every link, the remaining degree-2 pixels as cycles, and a sort."""
import numpy as np

CLOSED, HEAD_JUNCTION, TAIL_JUNCTION = 1, 2, 4
# the eight neighbours (dy, dx)
_N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
_DIAG = ((-1, -1), (-1, 1), (1, -1), (1, 1))


def foreground(mask):
    mask = np.asarray(mask)
    if mask.dtype == np.uint8:
        return mask != 0
    with np.errstate(invalid="ignore"):
        return mask > 0


def _shift(fg, dy, dx):
    """fg[y + dy, x + dx], False outside"""
    rows, cols = fg.shape
    out = np.zeros_like(fg)
    ys, yd = (slice(dy, rows), slice(0, rows - dy)) if dy >= 0 else (slice(0, rows + dy), slice(-dy, rows))
    xs, xd = (slice(dx, cols), slice(0, cols - dx)) if dx >= 0 else (slice(0, cols + dx), slice(-dx, cols))
    out[yd, xd] = fg[ys, xs]
    return out


def links(mask):
    """{(dy, dx): bool plane}: the pixel is linked to its neighbour at (dy, dx)"""
    fg = foreground(mask)
    out = {}
    for dy, dx in _N4:
        out[(dy, dx)] = fg & _shift(fg, dy, dx)
    for dy, dx in _DIAG:
        out[(dy, dx)] = fg & _shift(fg, dy, dx) & ~_shift(fg, dy, 0) & ~_shift(fg, 0, dx)
    return out


def adjacency(mask):
    """lin -> sorted list of the lin of its linked pixels, for every foreground pixel"""
    fg = foreground(mask)
    rows, cols = fg.shape
    adj = {int(p): [] for p in np.flatnonzero(fg)}
    for (dy, dx), plane in links(mask).items():
        for p in np.flatnonzero(plane):
            adj[int(p)].append(int(p) + dy * cols + dx)
    for v in adj.values():
        v.sort()
    return adj


def trace(mask):
    """list of (pixels as lin, flags) in the contract's order, and the adjacency"""
    adj = adjacency(mask)
    node = {p for p, v in adj.items() if len(v) != 2}
    chains = []
    used = set()   # directed steps taken from a node, so that every open chain is walked once from each end and listed once
    for p0 in sorted(node):
        if not adj[p0]:
            chains.append(((p0, -1), [p0], 0))
            continue
        for p1 in adj[p0]:
            if (p0, p1) in used:
                continue
            path = [p0, p1]
            while path[-1] not in node:
                a, b = adj[path[-1]]
                path.append(b if a == path[-2] else a)
            used.add((p0, p1))
            used.add((path[-1], path[-2]))
            fwd, bwd = (path[0], path[1]), (path[-1], path[-2])
            assert fwd != bwd
            if bwd < fwd:
                path.reverse()
            flags = (HEAD_JUNCTION if len(adj[path[0]]) >= 3 else 0) | (TAIL_JUNCTION if len(adj[path[-1]]) >= 3 else 0)
            chains.append(((path[0], path[1]), path, flags))
    seen = set()
    for _, path, _ in chains:
        seen.update(path)
    for p0 in sorted(adj):   # what is left has degree 2 throughout: cycles, each from its smallest pixel towards the smaller neighbour
        if p0 in seen:
            continue
        path = [p0, adj[p0][0]]
        while True:
            a, b = adj[path[-1]]
            nxt = b if a == path[-2] else a
            if nxt == p0:
                break
            path.append(nxt)
        seen.update(path)
        chains.append(((path[0], path[1]), path, CLOSED))
    chains.sort(key=lambda c: c[0])
    return [(path, flags) for _, path, flags in chains], adj


def chains(mask):
    """cvs_contour_chains: (points (N, 2) int32 of (x, y), table (M, 4) int32 of (start, length, flags, 0))"""
    cols = np.asarray(mask).shape[1]
    listed, _ = trace(mask)
    pts, table, start = [], [], 0
    for path, flags in listed:
        table.append((start, len(path), flags, 0))
        pts.extend((p % cols, p // cols) for p in path)
        start += len(path)
    return np.array(pts, np.int32).reshape(-1, 2), np.array(table, np.int32).reshape(-1, 4)
