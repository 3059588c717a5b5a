"""CPU test: the model of cvs_chain_paths (paths_model.py) against expectations derived by hand on small masks -- which chains each path
holds, in which order and direction, where its points start -- and the header, the binding and the build lists of the new call.  The
join tables come from joins_model over chains_model, radius 8, min_arm 3, min_cos -1 unless a test says otherwise."""
import os
import re

import numpy as np

import chains_model as CM
import joins_model as JM
import paths_model as M
import turns_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CFG = dict(radius=8, min_arm=3, min_cos=-1.0)


def junction_mask():
    """the plus, the T and the diagonal X of tests/test_gpu_joins.py: 9 x 9 each, side by side on the 33 x 65 plane"""
    mask = np.zeros((33, 65), F32)
    mask[6, 2:11], mask[2:11, 6] = 1, 1
    mask[14, 20:29], mask[14:23, 24] = 1, 1
    for k in range(9):
        mask[20 + k, 40 + k], mask[20 + k, 48 - k] = 1, 1
    return mask


def ring4_mask():
    """a square ring with a spur outwards from the middle of each side: four ring pieces between four T junctions"""
    mask = np.zeros((33, 65), F32)
    mask[8, 8:21], mask[20, 8:21], mask[8:21, 8], mask[8:21, 20] = 1, 1, 1, 1
    mask[2:8, 14], mask[21:27, 14], mask[14, 2:8], mask[14, 21:27] = 1, 1, 1, 1
    return mask


def lollipop_mask():
    """a square ring and one stem: the ring is ONE chain that leaves the junction and comes back to it"""
    mask = np.zeros((33, 65), F32)
    mask[10, 5:16], mask[20, 5:16], mask[10:21, 5], mask[10:21, 15] = 1, 1, 1, 1
    mask[15, 15:30] = 1
    return mask


def random_mask(density):
    return (np.random.default_rng(int(100 * density)).random((64, 64)) < density).astype(F32)


def build(mask, **cfg):
    pts, chains = CM.chains(mask)
    pts, chains = np.asarray(pts, np.int32), np.asarray(chains, np.int32)
    joins = JM.joins(pts, chains, **dict(CFG, **cfg))
    return pts, chains, joins, M.paths(pts, chains, joins)


def members_of(r):
    """per path the list of (chain, reversed)"""
    return [[(int(m["chain"]), int(m["flags"])) for m in r["members"][i["first_member"]:i["first_member"] + i["n_members"]]] for i in r["info"]]


def check_points(pts, chains, r):
    """the points of every path, rebuilt from the member list alone: each member's points in its direction, the first dropped from the
    second member on, the last of a cycle dropped"""
    for p, (members, (start, length, flags, plane)) in enumerate(zip(members_of(r), r["paths"].tolist())):
        want = []
        for k, (c, rev) in enumerate(members):
            s, ln = int(chains[c, 0]), int(chains[c, 1])
            seg = pts[s:s + ln][::-1] if rev else pts[s:s + ln]
            assert int(r["members"][r["info"][p]["first_member"] + k]["start"]) == start + len(want)
            want += seg[1 if k else 0:].tolist()
        if r["cycles"][p]:
            assert want[-1] == want[0]                                           # the walk came back to its first pixel
            want = want[:-1]
        assert r["path_points"][start:start + length].tolist() == want, p
        assert plane == chains[members[0][0], 3]
    assert r["paths"][:, 0].tolist() == np.concatenate([[0], np.cumsum(r["paths"][:, 1])[:-1]]).tolist()   # the running-sum rule
    assert int(r["paths"][:, 1].sum()) == len(r["path_points"]) == r["counts"][1]
    assert np.array_equal(pts[r["index"]], r["path_points"])


# ---- header, binding and build ----
def test_header_binding_and_build_lists():
    text = open(os.path.join(ROOT, "include", "cvsteer_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int cvs_chain_paths\(([^;]*)\);", plain)
    assert m, "cvs_chain_paths is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "points", "n_points", "chains", "n_chains", "joins", "xy", "path_points", "paths",
                                                          "info", "members", "index", "path_xy", "counts", "mem"]
    assert re.search(r"typedef struct cvs_path_member \{[^}]*chain;[^}]*flags;[^}]*path;[^}]*start;[^}]*\} cvs_path_member;", plain, re.S)
    assert re.search(r"typedef struct cvs_path_info \{[^}]*first_member, n_members;[^}]*first_end, last_end;[^}]*\} cvs_path_info;", plain, re.S)
    assert "CVS_MEMBER_REVERSED = 1" in plain
    assert "left to the caller" not in text
    from cvsteer_amd import _lib as L
    import ctypes as C
    res, argtypes = L.SIGNATURES["cvs_chain_paths"]
    assert res is C.c_int and len(argtypes) == len(args) and argtypes[-1] is C.c_int
    assert L.MEMBER_REVERSED == M.MEMBER_REVERSED == 1
    assert C.sizeof(L.PathMember) == M.PATH_MEMBER_DTYPE.itemsize == 16 and C.sizeof(L.PathInfo) == M.PATH_INFO_DTYPE.itemsize == 16
    assert [n for n, _ in L.PathMember._fields_] == list(M.PATH_MEMBER_DTYPE.names)
    assert [n for n, _ in L.PathInfo._fields_] == list(M.PATH_INFO_DTYPE.names)
    make = open(os.path.join(ROOT, "cvsteer_amd", "csrc", "Makefile")).read()
    units = dict(re.findall(r"^(HOST_UNITS|KERNEL_UNITS)\s*=\s*(.*)$", make, re.M))
    assert "cvs_paths" in units["HOST_UNITS"].split() and "cvs_kernels_paths" in units["KERNEL_UNITS"].split()
    # the launch count and the scratch the header names are the ones the kernels' header computes
    hdr = open(os.path.join(ROOT, "cvsteer_amd", "csrc", "cvs_paths.h")).read()
    assert "kPathEndBytes = 80" in hdr and "CVS_PATH_SCRATCH_PER_END = 80" in plain and "return 2 * path_rounds(n_chains) + 8;" in hdr
    assert "2 * ceil(log2(n_chains)) + 8" in text


# ---- hand-derived structures ----
def test_plus_t_and_x():
    """11 chains.  The plus (centre (6, 6)): chains 0 (top arm, down to the centre), 1 (left arm, in to the centre), 2 (centre to the
    right), 3 (centre downwards); straight through are 0-3 and 1-2.  The T (junction (24, 14)): 4 (left arm, in), 5 (junction to the
    right), 6 (the stem, nine points, on its own).  The X (centre (44, 24)): 7 and 8 run into the centre from the upper left and upper
    right, 9 and 10 leave it to the lower left and lower right; straight through are 7-10 and 8-9.  Nothing is reversed: every arm that
    reaches a centre ends there and every arm that leaves one starts there."""
    pts, chains, joins, r = build(junction_mask())
    assert len(chains) == 11 and chains[:, 1].tolist() == [5, 5, 5, 5, 5, 5, 9, 5, 5, 5, 5]
    assert members_of(r) == [[(0, 0), (3, 0)], [(1, 0), (2, 0)], [(4, 0), (5, 0)], [(6, 0)], [(7, 0), (10, 0)], [(8, 0), (9, 0)]]
    assert r["walks"] == [[0, 6], [2, 4], [8, 10], [12], [14, 20], [16, 18]] and not any(r["cycles"])
    assert max(len(m) for m in members_of(r)) == 2                               # every multi-member path: a straight-through pair
    assert r["paths"].tolist() == [[0, 9, 0, 0], [9, 9, 0, 0], [18, 9, 0, 0], [27, 9, M.HEAD_JUNCTION, 0], [36, 9, 0, 0], [45, 9, 0, 0]]
    assert r["info"].tolist() == [(0, 2, 0, 7), (2, 2, 2, 5), (4, 2, 8, 11), (6, 1, 12, 13), (7, 2, 14, 21), (9, 2, 16, 19)]
    assert r["members"]["start"].tolist() == [0, 5, 9, 14, 18, 23, 27, 36, 41, 45, 50]
    assert r["counts"] == (6, 59 - 5)                                            # five linked pairs, each one junction pixel listed once
    for p in (0, 1, 2, 4, 5):                                                    # straight lines of nine pixels through the junction
        q = r["path_points"][r["paths"][p, 0]:r["paths"][p, 0] + 9]
        d = np.diff(q, axis=0)
        assert (d == d[0]).all()
    check_points(pts, chains, r)


def test_ring4():
    """8 chains: the spurs 0 (top), 3 (left), 5 (right), 7 (bottom) and the ring pieces 1, 2 (from the top junction (14, 8) to the left and
    to the right junction), 4, 6 (from the left and the right junction to the bottom one).  At every T the two ring pieces continue each
    other and the spur is left over, so the ring is ONE cycle.  Its smallest end is 2, the head of chain 1: 1 forward to the left
    junction, 4 forward to the bottom, 6 backwards up to the right, 2 backwards to the top -- 12 pixels each, 48 in all."""
    pts, chains, joins, r = build(ring4_mask())
    assert len(chains) == 8 and chains[:, 1].tolist() == [7, 13, 13, 7, 13, 7, 13, 7]
    assert members_of(r) == [[(0, 0)], [(1, 0), (4, 0), (6, 1), (2, 1)], [(3, 0)], [(5, 0)], [(7, 0)]]
    assert r["walks"][1] == [2, 8, 13, 5] and r["cycles"] == [False, True, False, False, False]
    twin = [e ^ 1 for e in reversed(r["walks"][1])]
    assert twin == [4, 12, 9, 3] and set(twin).isdisjoint(r["walks"][1])         # the walk and its twin are distinct
    assert r["paths"].tolist() == [[0, 7, M.TAIL_JUNCTION, 0], [7, 48, M.CLOSED, 0], [55, 7, M.TAIL_JUNCTION, 0], [62, 7, M.HEAD_JUNCTION, 0],
                                   [69, 7, M.HEAD_JUNCTION, 0]]
    assert r["info"].tolist() == [(0, 1, 0, 1), (1, 4, 2, 4), (5, 1, 6, 7), (6, 1, 10, 11), (7, 1, 14, 15)]
    assert r["members"]["start"].tolist() == [0, 7, 20, 32, 44, 55, 62, 69]
    ring = r["path_points"][7:55]
    assert len({tuple(p) for p in ring.tolist()}) == 48                         # every ring pixel once
    step = np.abs(np.diff(np.concatenate([ring, ring[:1]]), axis=0)).sum(axis=1)
    assert (step == 1).all()                                                     # and the cycle closes
    check_points(pts, chains, r)


def test_lollipop():
    """2 chains: the ring, 41 points from the junction (15, 15) round and back to it, and the stem of 15.  The ring's two ends are each
    other's partners (the stem's end at the junction meets them at right angles): one CLOSED path of one member with L - 1 = 40 points."""
    pts, chains, joins, r = build(lollipop_mask())
    assert chains[:, :2].tolist() == [[0, 41], [41, 15]]
    assert joins["partner"][[0, 1]].tolist() == [1, 0] and (joins["flags"][[0, 1]] == JM.MUTUAL).all()
    assert members_of(r) == [[(0, 0)], [(1, 0)]] and r["cycles"] == [True, False]
    assert r["paths"].tolist() == [[0, 40, M.CLOSED, 0], [40, 15, M.HEAD_JUNCTION, 0]]
    assert r["info"].tolist() == [(0, 1, 0, 1), (1, 1, 2, 3)] and r["members"]["start"].tolist() == [0, 40]
    assert np.array_equal(r["path_points"][:40], pts[:40]) and np.array_equal(pts[40], pts[0])
    check_points(pts, chains, r)


def test_random_masks_have_long_open_paths_and_cycles():
    longest, cycles = {}, {}
    for density in (0.2, 0.5):
        for min_arm in (1, 3):
            pts, chains, joins, r = build(random_mask(density), min_arm=min_arm)
            check_points(pts, chains, r)
            sizes = [len(w) for w in r["walks"]]
            longest[density, min_arm] = max(n for n, c in zip(sizes, r["cycles"]) if not c)
            cycles[density, min_arm] = sorted(n for n, c in zip(sizes, r["cycles"]) if c)
            assert sorted(c for m in members_of(r) for c, _ in m) == list(range(len(chains)))   # every chain in exactly one path
            assert r["info"]["first_end"].tolist() == sorted(r["info"]["first_end"].tolist())
            assert any(rev for m in members_of(r) for _, rev in m)
    assert longest[0.2, 1] == 7 and longest[0.5, 1] == 17 and cycles[0.2, 1] == cycles[0.5, 1] == []
    assert cycles[0.2, 3] == [1, 2, 2] and cycles[0.5, 3] == [1, 1, 2]          # both kinds occur


def test_identity_without_links():
    """a join table of all NONE: the outputs are the inputs"""
    for mask in (junction_mask(), random_mask(0.2)):
        pts, chains = (np.asarray(a, np.int32) for a in CM.chains(mask))
        none = np.zeros(2 * len(chains), JM.JOIN_DTYPE)
        none["node"] = none["next"] = none["partner"] = -1
        none["flags"] = JM.NONE
        r = M.paths(pts, chains, none)
        assert r["paths"].tobytes() == chains.tobytes() and r["path_points"].tobytes() == pts.tobytes()
        assert r["index"].tolist() == list(range(len(pts)))
        assert r["members"].tolist() == [(c, 0, c, int(chains[c, 0])) for c in range(len(chains))]
        assert r["info"].tolist() == [(c, 1, 2 * c, 2 * c + 1) for c in range(len(chains))]
        # a MUTUAL flag alone links nothing: the partner has to agree
        one_sided = none.copy()
        one_sided["flags"][::2] = JM.MUTUAL
        one_sided["partner"][::2] = np.arange(1, 2 * len(chains), 2)[::-1]
        assert M.paths(pts, chains, one_sided)["paths"].tobytes() == chains.tobytes()


def test_tables_of_any_bytes_end():
    """LINKED is total: random words, partners out of range, entries that are no chains"""
    rng = np.random.default_rng(7)
    pts, chains = (np.asarray(a, np.int32) for a in CM.chains(random_mask(0.2)))
    m = len(chains)
    words = rng.integers(-2 ** 31, 2 ** 31, (2 * m, 8), dtype=np.int64).astype(np.int32)
    r = M.paths(pts, chains, words)
    assert r["counts"][0] <= m and r["counts"][1] <= len(pts)
    dense = words.copy()
    dense[:, 3] = rng.integers(-2, 2 * m + 2, 2 * m)                             # partners mostly in range: some pairs agree by chance
    dense[:, 4] |= 1
    broken = chains.copy()
    broken[3, 0], broken[5, 1], broken[7, 1] = -1, 0, 2 ** 30
    r = M.paths(pts, broken, dense)
    assert sorted(set(r["members"]["chain"].tolist())) == [c for c in range(m) if c not in (3, 5, 7)]


# ---- the 120 degree ridge: the corner the chains hide ----
def test_ridge_of_120_degrees_is_one_path_with_its_corner():
    """Thinning cuts the ridge at its vertex (test_joins_cpu.py): chains 0 (19 points, into the vertex pixel (24, 24)), 1 (the spur of 3)
    and 2 (24 points, out of the vertex).  The two long chains are MUTUAL partners there, so they are one path of 19 + 24 - 1 = 42 points
    through the vertex pixel, which is path point 18; the spur stays a path of its own.  cvs_chain_turns finds no corner on the three
    chains.  On the path, as the turns model shows it (integer points): exactly ONE corner, at path point 18 = the vertex pixel, with
        radius 4: cos -0.40614     radius 5: cos -0.41906     radius 8: cos -0.43475      (sin 0.914 .. 0.901: one clockwise turn)
    -- at radius 4 and 8 the very cosine cvs_chain_joins gives the mutual join there, since both are the turn between the same arms."""
    img, theta, (vx, vy), mask = TM.ridge_case(0.0, 120.0)
    pts, chains, joins, r = build(mask)
    assert chains[:, :2].tolist() == [[0, 19], [19, 3], [22, 24]]
    assert members_of(r) == [[(0, 0), (2, 0)], [(1, 0)]]
    assert r["paths"].tolist() == [[0, 42, 0, 0], [42, 3, M.HEAD_JUNCTION, 0]] and r["members"]["start"].tolist() == [0, 19, 42]
    vertex = r["path_points"][18]
    assert vertex.tolist() == pts[18].tolist() == pts[22].tolist() == [24, 24] and np.hypot(vertex[0] - vx, vertex[1] - vy) <= 1.5
    check_points(pts, chains, r)
    assert not (TM.turns(pts, chains, radius=5)["flags"] & TM.CORNER).any()      # the chains hide it
    for radius, cos in ((4, -0.40614), (5, -0.41906), (8, -0.43475)):
        t = TM.turns(r["path_points"], r["paths"], radius=radius)
        corners = np.nonzero(t["flags"] & TM.CORNER)[0]
        assert corners.tolist() == [18] and abs(float(t["cos"][18]) - cos) < 1e-5 and t["sin"][18] > 0.9
        print("ridge of 120 degrees as one path, radius %d: corner at path point 18, cos %.5f sin %.5f" % (radius, t["cos"][18], t["sin"][18]))
        if radius in (4, 8):
            j = JM.joins(pts, chains, radius=radius, min_arm=3)
            assert t["cos"][18].tobytes() == j["cos"][1].tobytes()               # end 1: the tail of chain 0, at the vertex
