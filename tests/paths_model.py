"""Model of cvs_chain_paths (plain Python and numpy, no GPU): written from the contract in include/cvsteer_hip.h, not from the kernels.  It
imports nothing from the library.

Sequential throughout: the LINKED test on every end, then every walk followed one step at a time with a visited set -- no pointer
jumping, no ranking, no scan.  On every input it asserts that the two twins of a path are different walks, and the two count
identities of the contract."""
import numpy as np

PATH_MEMBER_DTYPE = np.dtype([("chain", "<i4"), ("flags", "<i4"), ("path", "<i4"), ("start", "<i4")])
PATH_INFO_DTYPE = np.dtype([("first_member", "<i4"), ("n_members", "<i4"), ("first_end", "<i4"), ("last_end", "<i4")])
CLOSED, HEAD_JUNCTION, TAIL_JUNCTION = 1, 2, 4
MUTUAL = 1
MEMBER_REVERSED = 1


def join_words(joins, n_chains):
    """(partner, flags) of the 2 * n_chains records, from the structured table of cvs_chain_joins or from its raw 32-byte records"""
    j = np.ascontiguousarray(joins)
    if j.dtype.names:
        return j["partner"].astype(np.int64).tolist(), j["flags"].astype(np.int64).tolist()
    w = j.reshape(-1).view(np.uint8).view("<i4").reshape(2 * n_chains, 8)
    return w[:, 3].astype(np.int64).tolist(), w[:, 4].astype(np.int64).tolist()


def _twin(walk):
    return [e ^ 1 for e in reversed(walk)]


def paths(points, chains, joins, xy=None):
    """what cvs_chain_paths writes, for any tables a DEVICE call accepts: a dict of path_points (P, 2) int32, paths (K, 4) int32, info and
    members (structured), index (P,) int32, path_xy ((P, 2) float32, or None without xy), counts (n_paths, n_path_points), and for the
    tests the walks themselves (`walks`: per path the list of entry ends) and `cycles` (which paths are cycles)."""
    pts = np.asarray(points, np.int32).reshape(-1, 2)
    ch = np.asarray(chains, np.int64).reshape(-1, 4).tolist()
    n_points, m = len(pts), len(ch)
    partner, jflags = join_words(joins, m) if m else ([], [])
    fxy = None if xy is None else np.asarray(xy, np.float32).reshape(-1, 2)

    valid = [S >= 0 and L >= 1 and S + L <= n_points for S, L, F, R in ch]
    has_ends = [valid[c] and ch[c][1] >= 2 and not (ch[c][2] & CLOSED) for c in range(m)]

    def linked(e):
        p = partner[e]
        return bool(has_ends[e >> 1] and (jflags[e] & MUTUAL) and 0 <= p < 2 * m and p != e and has_ends[p >> 1] and (jflags[p] & MUTUAL)
                    and partner[p] == e)

    def succ(e):
        return partner[e ^ 1] if linked(e ^ 1) else None

    def pred(e):                                       # the f with succ(f) == e: f ^ 1 is the partner of e
        return partner[e] ^ 1 if linked(e) else None

    # every walk, once per twin: from an end without predecessor, or (cycles) from the smallest end not yet seen
    seen, walks = set(), []                            # walks: (entry ends, is a cycle)
    for e0 in range(2 * m):
        if not has_ends[e0 >> 1] or e0 in seen:
            continue
        e, steps = e0, 0
        while pred(e) is not None and pred(e) != e0:   # back to the first end of the walk, or once round a cycle
            e, steps = pred(e), steps + 1
            assert steps <= 2 * m, "predecessors are unique: going back ends or returns"
        cycle = pred(e) is not None
        if cycle:
            e = e0                                     # e0 is the smallest end of its cycle: all smaller ones were seen
        walk = []
        while e is not None and e not in seen:
            seen.add(e)
            walk.append(e)
            e = succ(e)
        assert (e is None) != cycle and (not cycle or e == walk[0]), "a walk neither ends nor closes on its first end"
        walks.append((walk, cycle))
    by_first = {}
    for walk, cycle in walks:
        if cycle:
            k = walk.index(min(walk))
            walk = walk[k:] + walk[:k]
        by_first[(walk[0], cycle)] = walk
    canon = []
    for (first, cycle), walk in by_first.items():
        tw = _twin(walk)
        if cycle:
            k = tw.index(min(tw))
            tw = tw[k:] + tw[:k]
        assert tw != walk and set(tw).isdisjoint(walk), "twins are never the same walk"
        assert (tw[0], cycle) in by_first and by_first[(tw[0], cycle)] == tw, "the twin of a walk is a walk"
        if walk[0] < tw[0]:
            canon.append((walk, cycle))
    for c in range(m):
        if valid[c] and not has_ends[c]:
            canon.append(([2 * c], False))
    canon.sort(key=lambda wc: wc[0][0])

    out_pts, out_idx, prec, irec, mrec = [], [], [], [], []
    for p, (walk, cycle) in enumerate(canon):
        start = len(out_idx)
        irec.append((len(mrec), len(walk), walk[0], walk[-1] ^ 1))
        for k, e in enumerate(walk):
            S, L, F, R = ch[e >> 1]
            pos = list(range(S, S + L)) if e % 2 == 0 else list(range(S + L - 1, S - 1, -1))
            if k >= 1:
                pos = pos[1:]
            if cycle and k == len(walk) - 1:
                pos = pos[:-1]
            mrec.append((e >> 1, MEMBER_REVERSED if e & 1 else 0, p, len(out_idx)))
            out_idx += pos
        c0, cl = walk[0] >> 1, (walk[-1] ^ 1) >> 1
        if cycle or (ch[c0][2] & CLOSED):
            flags = CLOSED
        else:
            bit = lambda end: ch[end >> 1][2] & (TAIL_JUNCTION if end & 1 else HEAD_JUNCTION)
            flags = (HEAD_JUNCTION if bit(walk[0]) else 0) | (TAIL_JUNCTION if bit(walk[-1] ^ 1) else 0)
        prec.append((start, len(out_idx) - start, flags, ch[c0][3]))

    n_pairs = sum(linked(e) for e in range(2 * m)) // 2
    n_cycles = sum(1 for _, cycle in canon if cycle)
    assert len(out_idx) == sum(ch[c][1] for c in range(m) if valid[c]) - n_pairs, "n_path_points = points of valid entries - linked pairs"
    assert len(canon) == sum(valid) - n_pairs + n_cycles, "n_paths = valid entries - linked pairs + cycles"
    assert len(mrec) == sum(valid)

    index = np.asarray(out_idx, np.int32).reshape(-1)
    return {
        "path_points": pts[index].reshape(-1, 2),
        "paths": np.asarray(prec, np.int32).reshape(-1, 4),
        "info": np.array(irec, PATH_INFO_DTYPE),
        "members": np.array(mrec, PATH_MEMBER_DTYPE),
        "index": index,
        "path_xy": None if fxy is None else fxy[index].reshape(-1, 2),
        "counts": (len(canon), len(out_idx)),
        "walks": [w for w, _ in canon],
        "cycles": [c for _, c in canon],
    }


def same_bytes(name, got, want):
    """two arrays byte for byte, structured ones field by field first so that a failure names the field"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.dtype, want.shape)
    for f in got.dtype.names or ():
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, "%s.%s differs at %d position(s), the first %s: %s, not %s" % (
            name, f, len(bad), bad[:8].tolist(), got[f][bad[:4]].tolist(), want[f][bad[:4]].tolist())
    if got.tobytes() != want.tobytes():
        a, b = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
        bad = np.nonzero(a != b)[0]
        raise AssertionError("%s differs at %d byte(s), the first at element %s" % (name, len(bad), (bad[:8] // max(got.itemsize, 1)).tolist()))
    return True
