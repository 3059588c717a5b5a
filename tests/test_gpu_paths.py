"""GPU test (-m gpu): contour paths -- cvs_chain_paths, chain_paths / contour_paths and the facade's stitchContours against the sequential
model of paths_model.py.

Every byte of every output is held to the model: the call is integer arithmetic and copies, so there is no tolerance anywhere.  The
device path, the host path, the same call twice and a captured graph give the same bytes; tables the library did not write end the call
like any other, and nothing outside the arrays, and no record past the counts, is written."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import chains_model as CM
import cvsteer_amd as cv
import joins_model as JM
import paths_model as M
import polyline_model as PM
import refine_model as RM
import turns_model as TM
from cvsteer_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32 = np.float32
GUARD = 64
SENTINEL = 0x5A5A5A5A
CFG = dict(radius=8, min_arm=3, min_cos=-1.0)
_cache = {}


def _filters(shape=(33, 65)):
    if shape not in _cache:
        _cache[shape] = cv.SteerableFiltersG2(torch.zeros(shape, device=DEV))
    return _cache[shape]


def _up(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _junction_mask():
    """the plus, the T and the diagonal X of tests/test_gpu_joins.py"""
    mask = np.zeros((33, 65), F32)
    mask[6, 2:11], mask[2:11, 6] = 1, 1
    mask[14, 20:29], mask[14:23, 24] = 1, 1
    for k in range(9):
        mask[20 + k, 40 + k], mask[20 + k, 48 - k] = 1, 1
    return mask


def _ring4_mask():
    mask = np.zeros((33, 65), F32)
    mask[8, 8:21], mask[20, 8:21], mask[8:21, 8], mask[8:21, 20] = 1, 1, 1, 1
    mask[2:8, 14], mask[21:27, 14], mask[14, 2:8], mask[14, 21:27] = 1, 1, 1, 1
    return mask


def _lollipop_mask():
    mask = np.zeros((33, 65), F32)
    mask[10, 5:16], mask[20, 5:16], mask[10:21, 5], mask[10:21, 15] = 1, 1, 1, 1
    mask[15, 15:30] = 1
    return mask


def _jitter(pts):
    """the points plus a fixed sub-pixel jitter (that of the joins test)"""
    return (pts + np.random.default_rng(len(pts)).uniform(-0.4, 0.4, pts.shape)).astype(F32)


def _words(joins):
    """a join table as the (2M, 8) int32 words the C call reads"""
    return np.ascontiguousarray(joins).reshape(-1).view(np.uint8).view("<i4").reshape(-1, 8).copy()


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (points, chains, xy, join table as words): the join tables of the integer points, min_arm 3 and, on the random masks, 1"""
    masks = {"junctions": (_junction_mask(), 3), "ring4": (_ring4_mask(), 3), "lollipop": (_lollipop_mask(), 3),
             "ridge": (TM.ridge_case(0.0, 120.0)[3], 3)}
    for density in (0.2, 0.5):
        for min_arm in (1, 3):
            masks["random %.2f arm %d" % (density, min_arm)] = ((np.random.default_rng(int(100 * density)).random((64, 64)) < density).astype(F32), min_arm)
    out = {}
    for name, (mask, min_arm) in masks.items():
        pts, chains = (np.ascontiguousarray(np.asarray(a, np.int32)) for a in CM.chains(mask))
        arrays = (pts, chains, _jitter(pts), _words(JM.joins(pts, chains, **dict(CFG, min_arm=min_arm))))
        for a in arrays:
            a.setflags(write=False)
        out[name] = arrays
    return out


NAMES = ["junctions", "ring4", "lollipop", "ridge", "random 0.20 arm 1", "random 0.20 arm 3", "random 0.50 arm 1", "random 0.50 arm 3"]


@functools.lru_cache(maxsize=None)
def _want(name):
    pts, chains, xy, joins = _cases()[name]
    return M.paths(pts, chains, joins, xy)


def _as_dict(r, with_xy, with_index):
    """what chain_paths returned, as host arrays under the model's names"""
    host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    d = {"path_points": host(r[0]), "paths": host(r[1]), "members": r[2], "info": r[3]}
    k = 4
    if with_xy:
        d["path_xy"], k = host(r[k]), k + 1
    if with_index:
        d["index"] = host(r[k])
    return d


def _same(got, want, what):
    for key, g in got.items():
        M.same_bytes("%s: %s" % (what, key), g, want[key])


# ---- masks ----
@pytest.mark.parametrize("name", NAMES)
def test_masks_byte_for_byte(name):
    pts, chains, xy, joins = _cases()[name]
    want = _want(name)
    f = _filters()
    table = np.ascontiguousarray(joins).view(np.uint8).reshape(-1, 32)
    first = None
    for with_xy in (False, True):
        for with_index in (False, True):
            dev = f.chain_paths(_up(pts), _up(chains), _up(table), xy=_up(xy) if with_xy else None, return_index=with_index)
            assert all(t.is_cuda for t in (dev[0], dev[1])) and dev[0].dtype == dev[1].dtype == torch.int32
            assert dev[2].dtype == M.PATH_MEMBER_DTYPE and dev[3].dtype == M.PATH_INFO_DTYPE
            assert len(dev) == 4 + with_xy + with_index
            got = _as_dict(dev, with_xy, with_index)
            _same(got, want, "%s device xy=%s index=%s" % (name, with_xy, with_index))
            host = f.chain_paths(np.array(pts), np.array(chains), joins.view(JM.JOIN_DTYPE).reshape(-1), xy=np.array(xy) if with_xy else None,
                                 return_index=with_index)
            assert isinstance(host[0], np.ndarray)
            _same(_as_dict(host, with_xy, with_index), want, "%s host xy=%s index=%s" % (name, with_xy, with_index))
            again = _as_dict(f.chain_paths(_up(pts), _up(chains), _up(table), xy=_up(xy) if with_xy else None, return_index=with_index),
                             with_xy, with_index)
            assert all(again[k].tobytes() == got[k].tobytes() for k in got)        # the same call twice: the same bytes
            first = first or got
    assert (len(want["paths"]), len(want["path_points"])) == want["counts"] == (len(first["paths"]), len(first["path_points"]))
    if name == "junctions":                                                         # through the library's own chains and joins
        d_pts, d_chains = f.contour_chains(_up(_junction_mask()))
        assert np.array_equal(d_pts.cpu().numpy(), pts) and np.array_equal(d_chains.cpu().numpy(), chains)
        r = f.chain_paths(d_pts, d_chains, f.chain_joins(d_pts, d_chains, **CFG))   # (the structured table, uploaded by chain_paths)
        _same(_as_dict(r, False, False), want, "junctions, the library's own tables")
        assert [len(w) for w in want["walks"]] == [2, 2, 2, 1, 2, 2]
    if name == "ring4":
        assert want["cycles"] == [False, True, False, False, False] and want["walks"][1] == [2, 8, 13, 5]
    if name == "lollipop":
        assert first["paths"].tolist() == [[0, 40, M.CLOSED, 0], [40, 15, M.HEAD_JUNCTION, 0]]
    if name.startswith("random") and name.endswith("arm 3"):
        assert any(want["cycles"])
    if name == "random 0.50 arm 1":
        assert max(len(w) for w in want["walks"]) == 17 and not any(want["cycles"])


def test_identity_without_links():
    pts, chains, xy, _ = _cases()["random 0.20 arm 3"]
    none = np.zeros(2 * len(chains), JM.JOIN_DTYPE)
    none["node"] = none["next"] = none["partner"] = -1
    none["flags"] = JM.NONE
    f = _filters()
    got = _as_dict(f.chain_paths(_up(pts), _up(chains), none, xy=_up(xy), return_index=True), True, True)
    assert got["paths"].tobytes() == chains.tobytes() and got["path_points"].tobytes() == pts.tobytes() and got["path_xy"].tobytes() == xy.tobytes()
    assert got["index"].tolist() == list(range(len(pts)))
    assert got["members"].tolist() == [(c, 0, c, int(chains[c, 0])) for c in range(len(chains))]
    assert got["info"].tolist() == [(c, 1, 2 * c, 2 * c + 1) for c in range(len(chains))]


# ---- composition: joins -> paths on the device, and every chain call on the paths ----
def test_composition_on_the_device():
    pts, chains, xy, _ = _cases()["random 0.50 arm 1"]
    f = _filters()
    d_pts, d_chains, d_xy = _up(pts), _up(chains), _up(xy)
    n, m = len(pts), len(chains)
    cfg = dict(radius=8, min_arm=1, min_cos=-1.0)
    tab = torch.empty((2 * m, 32), dtype=torch.uint8, device=DEV)
    out = (torch.empty((n, 2), dtype=torch.int32, device=DEV), torch.empty((m, 4), dtype=torch.int32, device=DEV),
           torch.empty((m, 16), dtype=torch.uint8, device=DEV), torch.empty((m, 16), dtype=torch.uint8, device=DEV),
           torch.empty((n, 2), dtype=torch.float32, device=DEV), torch.empty((n,), dtype=torch.int32, device=DEV),
           torch.empty((2,), dtype=torch.int32, device=DEV))
    assert f.chain_joins(d_pts, d_chains, xy=d_xy, out=tab, **cfg) is tab           # never downloaded in between
    assert f.chain_paths(d_pts, d_chains, tab, xy=d_xy, return_index=True, out=out) is out
    want = M.paths(pts, chains, JM.joins(pts, chains, xy, **cfg), xy)
    k, q = out[6].cpu().tolist()
    assert (k, q) == want["counts"] and max(len(w) for w in want["walks"]) >= 10
    p_pts, p_tab, p_xy = out[0][:q], out[1][:k], out[4][:q]
    M.same_bytes("path_points", p_pts.cpu().numpy(), want["path_points"])
    M.same_bytes("paths", p_tab.cpu().numpy(), want["paths"])
    M.same_bytes("path_xy", p_xy.cpu().numpy(), want["path_xy"])
    M.same_bytes("index", out[5][:q].cpu().numpy(), want["index"])
    M.same_bytes("info", out[3][:k].cpu().numpy().view(M.PATH_INFO_DTYPE).reshape(-1), want["info"])
    M.same_bytes("members", out[2][:len(want["members"])].cpu().numpy().view(M.PATH_MEMBER_DTYPE).reshape(-1), want["members"])
    # (path_points, paths) is a chain table like any other: the chain calls on whole contours, against their models on the model's paths
    w_pts, w_tab, w_xy = want["path_points"], want["paths"], want["path_xy"]
    assert not JM.host_table_wrong(len(w_pts), w_tab)                               # the running-sum rule
    for sub_d, sub_h in ((None, None), (p_xy, w_xy)):
        assert TM.same_records(f.chain_turns(p_pts, p_tab, xy=sub_d, radius=5), TM.turns(w_pts, w_tab, xy=sub_h, radius=5))
    for eps in (0.0, 1.0):
        got = f.chain_polylines(p_pts, p_tab, eps, return_index=True)
        for g, w in zip(got, PM.polylines(w_pts, w_tab, eps)):
            assert np.array_equal(g.cpu().numpy(), w)
    rec = f.chain_measures(p_pts, p_tab, xy=p_xy)
    model, _, abs_len = RM.measures(w_pts, w_tab, None, w_xy, return_abs=True)
    for field in ("axial", "diagonal", "other", "peak_index"):                      # the integer fields: exactly
        assert np.array_equal(rec[field], model[field]), field
    # (the length is a sum of square roots whose order of additions the measures contract leaves open: the bound of test_gpu_refine.py)
    assert (np.abs(rec["length"] - model["length"]) <= (w_tab[:, 1] + 2) * 2.0 ** -52 * abs_len).all()
    assert rec.tobytes() == f.chain_measures(_up(w_pts), _up(w_tab), xy=_up(w_xy)).tobytes()   # and the same bytes as on the model's arrays
    joins_again = f.chain_joins(p_pts, p_tab, xy=p_xy, **cfg)                       # the paths go through cvs_chain_joins itself
    assert JM.same_records(joins_again, JM.joins(w_pts, w_tab, w_xy, **cfg))


# ---- synthetic walks: more rounds than ten, a cycle cut far from its members ----
def _none_table(m):
    t = np.zeros((2 * m, 8), np.int32)
    t[:, [0, 2, 3]] = -1
    t[:, 4] = JM.NONE
    t[:, 6:] = JM.QNAN_BITS
    return t


def _link(t, e, f):
    t[e, 3], t[f, 3] = f, e
    t[e, 4] = t[f, 4] = JM.MUTUAL


def _long_walks(seed=11):
    """one closed polygonal walk (the outline of a 1000 x 300 rectangle, 2600 unit steps) as 1300 chains of 3 points, the chain numbers
    shuffled and every chain stored in a random direction; joined into an open path of the first 1000 and a cycle of the last 300"""
    corners = [(0, 0), (1000, 0), (1000, 300), (0, 300), (0, 0)]
    walk = [corners[0]]
    for (x0, y0), (x1, y1) in zip(corners[:-1], corners[1:]):
        steps = max(abs(x1 - x0), abs(y1 - y0))
        walk += [(x0 + (x1 - x0) * k // steps, y0 + (y1 - y0) * k // steps) for k in range(1, steps + 1)]
    assert len(walk) == 2601 and walk[0] == walk[-1]
    rng = np.random.default_rng(seed)
    m = 1300
    number, flipped = rng.permutation(m), rng.integers(0, 2, m)
    pts = np.zeros((3 * m, 2), np.int32)
    for i in range(m):
        three = walk[2 * i:2 * i + 3]
        pts[3 * number[i]:3 * number[i] + 3] = three[::-1] if flipped[i] else three
    chains = np.int32([[3 * c, 3, 0, 0] for c in range(m)])
    entry = lambda i: 2 * int(number[i]) + int(flipped[i])
    table = _none_table(m)
    for i in list(range(0, 999)) + list(range(1000, 1299)):
        _link(table, entry(i) ^ 1, entry(i + 1))
    _link(table, entry(1299) ^ 1, entry(1000))
    return pts, chains, table, number, flipped


def test_long_walks_and_the_smallest_tables():
    f = _filters()
    pts, chains, table, number, flipped = _long_walks()
    want = M.paths(pts, chains, table, _jitter(pts))
    sizes = sorted(len(w) for w in want["walks"])
    assert sizes == [300, 1000] and sorted(want["cycles"]) == [False, True] and want["counts"] == (2, 3 * 1300 - 1299)
    cyc = want["walks"][want["cycles"].index(True)]
    assert cyc[0] == min(min(cyc), min(e ^ 1 for e in cyc)) and cyc[0] % 2 == 0     # cut at the smallest end of both twins: a head
    for with_xy in (True, False):
        xy = _jitter(pts) if with_xy else None
        got = _as_dict(f.chain_paths(_up(pts), _up(chains), _up(table.view(np.uint8)), xy=_up(xy), return_index=True), with_xy, True)
        _same(got, want, "long walks, device")
        host = _as_dict(f.chain_paths(pts, chains, table.view(np.uint8), xy=xy, return_index=True), with_xy, True)
        _same(host, want, "long walks, host")
    # the open path runs along the outline: unit steps all the way, in one of its two directions
    p = want["cycles"].index(False)
    s, ln = want["paths"][p, :2]
    assert ln == 2001 and (np.abs(np.diff(got["path_points"][s:s + ln], axis=0)).sum(axis=1) == 1).all()
    # one chain, two chains, and a single chain whose two ends are partners
    one_p, one_c = np.int32([[4, 4], [5, 4], [6, 5]]), np.int32([[0, 3, 0, 0]])
    two_p, two_c = np.int32([[0, 0], [1, 0], [2, 0], [4, 2], [3, 1], [2, 0]]), np.int32([[0, 3, 0, 0], [3, 3, 0, 0]])
    loop, pair, apart = _none_table(1), _none_table(2), _none_table(2)
    _link(loop, 0, 1)
    _link(pair, 1, 3)                                                               # tail to tail: the second chain runs backwards
    for what, p_, c_, t_, paths_, members_ in (
            ("one chain", one_p, one_c, _none_table(1), [[0, 3, 0, 0]], [(0, 0, 0, 0)]),
            ("one chain, a loop", one_p, one_c, loop, [[0, 2, M.CLOSED, 0]], [(0, 0, 0, 0)]),
            ("two chains", two_p, two_c, apart, [[0, 3, 0, 0], [3, 3, 0, 0]], [(0, 0, 0, 0), (1, 0, 1, 3)]),
            ("two chains, joined", two_p, two_c, pair, [[0, 5, 0, 0]], [(0, 0, 0, 0), (1, M.MEMBER_REVERSED, 0, 3)])):
        want = M.paths(p_, c_, t_)
        assert want["paths"].tolist() == paths_ and want["members"].tolist() == members_, what
        for put in (_up, np.array):
            got = _as_dict(f.chain_paths(put(p_), put(c_), put(t_.view(np.uint8)), return_index=True), False, True)
            _same(got, want, what)
    assert got["path_points"].tolist() == [[0, 0], [1, 0], [2, 0], [3, 1], [4, 2]]


def test_batch_table_keeps_the_plane_of_the_first_member():
    f = _filters()
    a, b = _junction_mask(), _ring4_mask()
    pts, chains, ranges = f.contour_chains_batch(_up(np.stack([a, b])))
    h_pts, h_chains = pts.cpu().numpy(), chains.cpu().numpy()
    assert sorted(set(h_chains[:, 3].tolist())) == [0, 1]
    tab = torch.empty((2 * len(h_chains), 32), dtype=torch.uint8, device=DEV)
    f.chain_joins(pts, chains, out=tab, **CFG)
    want = M.paths(h_pts, h_chains, JM.joins(h_pts, h_chains, **CFG))
    got = _as_dict(f.chain_paths(pts, chains, tab, return_index=True), False, True)
    _same(got, want, "two planes")
    first = got["members"]["chain"][got["info"]["first_member"]]
    assert np.array_equal(got["paths"][:, 3], h_chains[first, 3]) and sorted(set(got["paths"][:, 3].tolist())) == [0, 1]
    for p, i in enumerate(got["info"]):                                             # no path leaves its plane
        assert len(set(h_chains[got["members"]["chain"][i["first_member"]:i["first_member"] + i["n_members"]], 3].tolist())) == 1, p
    assert (got["paths"][:, 2] == M.CLOSED).sum() == 1                              # the ring of the second plane


# ---- raw calls: guarded arrays, tables the library did not write, errors ----
def _guarded(n, words, fill=SENTINEL):
    """(buffer, view): n records of `words` int32 words with GUARD records of sentinel in front and behind, the records themselves sentinel too"""
    buf = torch.full((GUARD + n + GUARD, words), fill, dtype=torch.int32, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _ptr(a):
    return None if a is None else C.c_void_p(a if isinstance(a, int) else (a.data_ptr() if torch.is_tensor(a) else a.ctypes.data))


OUTS = (("path_points", 2, "n"), ("paths", 4, "m"), ("info", 4, "m"), ("members", 4, "m"), ("index", 1, "n"), ("path_xy", 2, "n"), ("counts", 1, 2))


def _raw(f, pts, n, chains, m, joins, xy, outs, mem):
    """cvs_chain_paths with the outputs of the dict `outs` (absent: NULL)"""
    o = lambda k: _ptr(outs.get(k))
    return L.lib().cvs_chain_paths(f._h, _ptr(pts), n, _ptr(chains), m, _ptr(joins), _ptr(xy), o("path_points"), o("paths"), o("info"),
                                   o("members"), o("index"), o("path_xy"), o("counts"), mem)


def _guarded_run(f, pts, chains, table, xy, what):
    """a DEVICE call into guarded outputs: returns the results trimmed to the counts after checking that the guards, the records past the
    counts and the inputs are untouched"""
    n, m = len(pts), len(chains)
    bufs = {k: _guarded(n if size == "n" else m if size == "m" else size, words) for k, words, size in OUTS}
    inputs = [torch.cat([torch.full((GUARD,) + a.shape[1:], 77, dtype=a.dtype, device=DEV), a, torch.full((GUARD,) + a.shape[1:], 77, dtype=a.dtype, device=DEV)])
              for a in (_up(pts), _up(chains), _up(table), _up(xy))]
    before = [a.clone() for a in inputs]
    gp, gc, gj, gx = (a[GUARD:len(a) - GUARD] for a in inputs)
    f._bind_stream(gp)
    assert _raw(f, gp, n, gc, m, gj, gx, {k: v[1] for k, v in bufs.items()}, L.MEM_DEVICE) == 0, what
    torch.cuda.synchronize()                                                        # the call returns, and so does the device
    assert all(torch.equal(a, b) for a, b in zip(inputs, before)), what             # no input is written
    host = {k: v[0].cpu().numpy() for k, v in bufs.items()}
    k, q = host["counts"][GUARD:GUARD + 2, 0].tolist()
    got = {}
    for key, words, size in OUTS:
        rows = n if size == "n" else m if size == "m" else size
        body = host[key][GUARD:GUARD + rows]
        used = {"path_points": q, "index": q, "path_xy": q, "paths": k, "info": k, "counts": 2}.get(key)
        if key == "members":
            used = int(host["info"][GUARD:GUARD + k, 1].sum())                     # every valid chain is one member
        assert (host[key][:GUARD] == SENTINEL).all() and (host[key][GUARD + rows:] == SENTINEL).all(), (what, key)
        assert (body[used:].view(np.uint32) == SENTINEL).all(), (what, key, "written past the counts")
        got[key] = body[:used]
    return {"path_points": got["path_points"], "paths": got["paths"], "info": got["info"].view(M.PATH_INFO_DTYPE).reshape(-1),
            "members": got["members"].view(M.PATH_MEMBER_DTYPE).reshape(-1), "index": got["index"].reshape(-1),
            "path_xy": got["path_xy"].view(F32), "counts": (k, q)}


def test_tables_the_library_did_not_write():
    pts, chains, xy, good = _cases()["random 0.20 arm 1"]
    n, m = len(pts), len(chains)
    f = _filters()
    rng = np.random.default_rng(3)
    linked = np.nonzero(good[:, 4] & JM.MUTUAL)[0]
    assert len(linked) >= 40
    cases = {}
    t = good.copy()                                                                 # partners out of range, on both sides of a pair and on one
    t[linked[0], 3], t[linked[2], 3], t[linked[4], 3], t[linked[6], 3] = -1, 2 * m, 2 ** 31 - 1, -2 ** 31
    cases["partners out of range"] = (chains, t)
    t = good.copy()
    t[linked[:10], 3] = linked[:10]                                                 # partner == own end
    cases["partner is the end itself"] = (chains, t)
    t = good.copy()
    t[linked[::3], 4] &= ~JM.MUTUAL                                                 # one-sided MUTUAL
    t[np.nonzero((good[:, 4] & JM.MUTUAL) == 0)[0][:50], 4] |= JM.MUTUAL            # and MUTUAL on ends whose partner does not agree
    cases["one-sided MUTUAL"] = (chains, t)
    c = chains.copy()                                                               # partner chains that are closed, too short or invalid
    hit = (good[linked[:12], 3] >> 1)
    c[hit[0:4], 2] |= M.CLOSED
    c[hit[4:8], 1] = 1
    c[hit[8:10], 0], c[hit[10:12], 1] = -5, 0
    cases["partner chains without ends"] = (c, good.copy())
    c = chains.copy()                                                               # invalid entries: S < 0, L < 1, S + L > n_points
    c[3, 0], c[5, 0], c[4, 1], c[6, 1], c[-1, 1], c[9, 1] = -1, -2 ** 31, 0, -3, c[-1, 1] + 1, 2 ** 31 - 1
    cases["invalid entries"] = (c, good.copy())
    cases["random words"] = (chains, rng.integers(-2 ** 31, 2 ** 31, (2 * m, 8), dtype=np.int64).astype(np.int32))
    t = rng.integers(-2 ** 31, 2 ** 31, (2 * m, 8), dtype=np.int64).astype(np.int32)
    t[:, 3] = rng.integers(-2, 2 * m + 2, 2 * m)                                    # random partners that are mostly ends, all MUTUAL
    t[:, 4] |= JM.MUTUAL
    cases["random partners"] = (chains, t)
    involution = rng.permutation(2 * m).reshape(-1, 2)                              # every end paired off at random: long walks
    t = _none_table(m)
    for e, g in involution.tolist():
        _link(t, e, g)
    cases["a random pairing of all ends"] = (chains, t)
    open_ = np.nonzero((chains[:, 1] >= 2) & ((chains[:, 2] & M.CLOSED) == 0))[0]     # the same among the chains that have ends: cycles only
    ends = rng.permutation(np.concatenate([2 * open_, 2 * open_ + 1]))
    t = _none_table(m)
    for e, g in ends.reshape(-1, 2).tolist():
        _link(t, e, g)
    cases["a random pairing of the ends that exist"] = (chains, t)
    seen_cycle = False
    for what, (tab, joins) in cases.items():
        want = M.paths(pts, tab, joins, xy)
        assert want["counts"][1] <= n                                               # (no entry was made longer: the points fit)
        got = _guarded_run(f, pts, tab, joins, xy, what)
        assert got["counts"] == want["counts"], what
        for key in ("path_points", "paths", "info", "members", "index", "path_xy"):
            M.same_bytes("%s: %s" % (what, key), got[key], want[key])
        seen_cycle |= any(want["cycles"])
    assert seen_cycle
    want = M.paths(pts, chains, cases["a random pairing of the ends that exist"][1], xy)
    assert all(c for c, w in zip(want["cycles"], want["walks"]) if len(w) > 1) and max(len(w) for w in want["walks"]) > 64


def test_errors_leave_the_outputs_untouched():
    pts, chains, xy, joins = _cases()["random 0.20 arm 3"]
    f = _filters()
    dp, dc, dx, dj = (_up(a) for a in (pts, chains, xy, joins))
    n, m, D, H, B = len(pts), len(chains), L.MEM_DEVICE, L.MEM_HOST, L.E_BADARG
    f._bind_stream(dp)
    outs = {k: torch.full(((n if size == "n" else m if size == "m" else size) + 1, words), -9, dtype=torch.int32, device=DEV) for k, words, size in OUTS}
    call = lambda p=dp, n_=n, c=dc, m_=m, j=dj, x=dx, mem=D, **change: _raw(f, p, n_, c, m_, j, x, {k: v for k, v in dict(outs, **change).items() if v is not None}, mem)
    # counts, arrays, mem
    assert call(n_=-1) == B and call(m_=-1) == B
    assert call(p=None) == B and call(c=None) == B and call(j=None) == B
    for key in ("path_points", "paths", "info", "members", "counts"):
        assert call(**{key: None}) == B, key
    assert call(path_xy=None) == B and call(x=None) == B                            # path_xy without xy, xy without path_xy
    assert call(c=None, m_=0) == B                                                  # points without a chain
    assert call(mem=5) == B and call(mem=-1) == B
    assert call(p=dp.data_ptr() + 2) == B and call(c=dc.data_ptr() + 2) == B and call(j=dj.data_ptr() + 2) == B and call(x=dx.data_ptr() + 2) == B
    for key in outs:                                                                # not aligned to 4 bytes
        assert call(**{key: outs[key].data_ptr() + 2}) == B, key
    for key in outs:                                                                # an output over an input, an output over another output
        for a in (dp, dc, dj, dx):
            assert call(**{key: a}) == B, key
        other = "paths" if key != "paths" else "info"
        assert call(**{key: outs[other]}) == B, key
    assert call(counts=outs["paths"].data_ptr() + 16 * m - 4) == B                  # the counts on the last word of paths
    assert call(n_=2 ** 30 + 1) == L.E_SIZE and call(m_=2 ** 26 + 1) == L.E_SIZE
    # host tables that do not say what the contract says
    h_outs = {k: np.full(tuple(v.shape), -9, np.int32) for k, v in outs.items()}
    host = lambda c, m_=m, p=np.array(pts), n_=n: _raw(f, p, n_, np.ascontiguousarray(c), m_, np.array(joins), np.array(xy), h_outs, H)
    for row, col, delta in ((-1, 1, 1), (-1, 1, -1), (0, 0, -1), (0, 0, 1), (1, 0, 1), (m // 2, 1, -int(chains[m // 2, 1]))):
        bad = np.array(chains)
        bad[row, col] += delta
        assert host(bad) == B, (row, col, delta)
    assert host(chains[:-1], m - 1) == B
    torch.cuda.synchronize()
    assert all(bool((v == -9).all()) for v in outs.values()) and all((v == -9).all() for v in h_outs.values())
    # n_chains == 0: counts = (0, 0), on both paths
    assert call(p=None, n_=0, c=None, m_=0, j=None) == 0 and host(chains[:0], 0, None, 0) == 0
    torch.cuda.synchronize()
    assert outs["counts"][:2, 0].tolist() == [0, 0] and int(outs["counts"][2, 0]) == -9 and h_outs["counts"][:2, 0].tolist() == [0, 0]
    assert all(bool((v == -9).all()) for k, v in outs.items() if k != "counts")
    # the same arrays unharmed: the calls go through, also into arrays that are aligned to 4 bytes only
    want = _want("random 0.20 arm 3")
    assert host(chains) == 0
    k, q = want["counts"]
    assert h_outs["counts"][:2, 0].tolist() == [k, q] and h_outs["paths"][:k].tobytes() == want["paths"].tobytes()
    assert h_outs["path_points"][:q].tobytes() == want["path_points"].tobytes() and (h_outs["path_points"][q:] == -9).all()   # nothing past the counts
    assert (h_outs["paths"][k:] == -9).all() and (h_outs["info"][k:] == -9).all() and (h_outs["index"][q:] == -9).all()
    flat = torch.full((4 * m + 8,), -9, dtype=torch.int32, device=DEV)
    assert call(paths=flat.data_ptr() + 4) == 0
    torch.cuda.synchronize()
    assert flat[1:1 + 4 * k].cpu().numpy().tobytes() == want["paths"].tobytes() and int(flat[0]) == -9 and bool((flat[1 + 4 * k:] == -9).all())


# ---- capture ----
def test_graph_capture():
    pts, chains, xy, _ = _cases()["random 0.20 arm 1"]
    n, m = len(pts), len(chains)
    cfg = dict(radius=8, min_arm=1, min_cos=-1.0)
    rough = (pts + np.random.default_rng(99).uniform(-3.0, 3.0, pts.shape)).astype(F32)   # other positions: other arms, other joins
    wants = [M.paths(pts, chains, JM.joins(pts, chains, sub, **cfg), sub) for sub in (xy, rough)]
    assert wants[0]["paths"].tobytes() != wants[1]["paths"].tobytes()
    d_pts, d_chains, d_xy = _up(pts), _up(chains), _up(xy)
    shapes = (((n, 2), torch.int32), ((m, 4), torch.int32), ((m, 16), torch.uint8), ((m, 16), torch.uint8), ((n, 2), torch.float32), ((2,), torch.int32))
    new_out = lambda: tuple(torch.zeros(sh, dtype=dt, device=DEV) for sh, dt in shapes)
    side = torch.cuda.Stream()
    # a first call under capture, on a handle whose scratch is cold: refused, and the handle works on
    cold = cv.SteerableFiltersG2(torch.zeros((33, 65), device=DEV))
    good = torch.from_numpy(_words(JM.joins(pts, chains, xy, **cfg)).view(np.uint8)).to(DEV)
    out = new_out()
    marker = torch.ones((4,), dtype=torch.int32, device=DEV)
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        cold._bind_stream(d_pts)
        torch.cuda.synchronize()
        with torch.cuda.graph(g0, stream=side):
            marker.zero_()                                                          # (so that the capture holds a node)
            rc = L.lib().cvs_chain_paths(cold._h, _ptr(d_pts), n, _ptr(d_chains), m, _ptr(good), _ptr(d_xy), _ptr(out[0]), _ptr(out[1]), _ptr(out[3]),
                                         _ptr(out[2]), None, _ptr(out[4]), _ptr(out[5]), L.MEM_DEVICE)
            message = L.lib().cvs_last_error(cold._h)
            hp, hc, hj = np.int32([[0, 0], [1, 0]]), np.int32([[0, 2, 0, 0]]), _none_table(1)
            ho = [np.full(s, -9, np.int32) for s in ((2, 2), (1, 4), (1, 4), (1, 4), (2,))]
            rc_host = L.lib().cvs_chain_paths(cold._h, _ptr(hp), 2, _ptr(hc), 1, _ptr(hj), None, _ptr(ho[0]), _ptr(ho[1]), _ptr(ho[2]), _ptr(ho[3]),
                                              None, None, _ptr(ho[4]), L.MEM_HOST)
    assert rc == L.E_UNSUPPORTED and b"call once eagerly first" in message
    assert rc_host == L.E_UNSUPPORTED and all((a == -9).all() for a in ho)
    torch.cuda.synchronize()
    assert all(not bool(t.any()) for t in out)
    got = _as_dict(cold.chain_paths(d_pts, d_chains, good, xy=d_xy), True, False)
    _same(got, wants[0], "the handle works on")
    # joins -> paths captured once, replayed on changed inputs of the same sizes
    f = cv.SteerableFiltersG2(torch.zeros((33, 65), device=DEV))
    tab = torch.empty((2 * m, 32), dtype=torch.uint8, device=DEV)
    out = new_out()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f.chain_joins(d_pts, d_chains, xy=d_xy, out=tab, **cfg)                     # once eagerly: the scratch gets its size
        f.chain_paths(d_pts, d_chains, tab, xy=d_xy, out=out)
        torch.cuda.synchronize()
        for t in out:
            t.zero_()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            f.chain_joins(d_pts, d_chains, xy=d_xy, out=tab, **cfg)
            assert f.chain_paths(d_pts, d_chains, tab, xy=d_xy, out=out) is out
    torch.cuda.synchronize()
    assert all(not bool(t.any()) for t in out)                                      # a capture runs nothing
    for sub, want in ((rough, wants[1]), (xy, wants[0])):
        d_xy.copy_(_up(sub))
        g.replay()
        torch.cuda.synchronize()
        k, q = out[5].cpu().tolist()
        assert (k, q) == want["counts"]
        M.same_bytes("paths", out[1][:k].cpu().numpy(), want["paths"])
        M.same_bytes("path_points", out[0][:q].cpu().numpy(), want["path_points"])
        M.same_bytes("path_xy", out[4][:q].cpu().numpy(), want["path_xy"])
        M.same_bytes("info", out[3][:k].cpu().numpy().view(M.PATH_INFO_DTYPE).reshape(-1), want["info"])
        M.same_bytes("members", out[2][:len(want["members"])].cpu().numpy().view(M.PATH_MEMBER_DTYPE).reshape(-1), want["members"])
        eager = _as_dict(f.chain_paths(d_pts, d_chains, f.chain_joins(d_pts, d_chains, xy=d_xy, **cfg), xy=d_xy), True, False)
        _same(eager, want, "eager")


# ---- end to end ----
def test_contour_paths_on_the_ridge_of_120_degrees():
    """the two arms of the ridge are one path through the vertex pixel, and cvs_chain_turns finds the corner there"""
    img, theta, (vx, vy), mask = TM.ridge_case(0.0, 120.0)
    f = cv.SteerableFiltersG2(_up(img))
    pts, chains = CM.chains(mask)
    xy, _ = RM.refine(pts, img, theta)
    want = M.paths(pts, chains, JM.joins(pts, chains, xy, radius=8), xy)
    r = f.contour_paths(_up(mask), _up(img), theta=_up(theta), radius=8)
    assert len(r) == 5 and r[0].is_cuda
    _same(_as_dict(r, True, False), want, "contour_paths")
    host = f.contour_paths(mask, img, theta=theta, radius=8)
    assert isinstance(host[0], np.ndarray)
    _same(_as_dict(host, True, False), want, "contour_paths, host")
    assert want["paths"][:, :2].tolist() == [[0, 42], [42, 3]] and want["path_points"][18].tolist() == [24, 24]
    assert not (f.chain_turns(_up(pts), _up(chains), radius=5)["flags"] & L.TURN_CORNER).any()
    turns = f.chain_turns(r[0], r[1], radius=5)
    assert TM.same_records(turns, TM.turns(want["path_points"], want["paths"], radius=5))
    assert np.nonzero(turns["flags"] & L.TURN_CORNER)[0].tolist() == [18] and -0.6 < turns["cos"][18] < -0.3
    with pytest.raises(ValueError):
        f.chain_paths(r[0], r[1], torch.zeros((3, 32), dtype=torch.uint8, device=DEV))


# ---- facade ----
def test_facade_member(tmp_path):
    exe = os.path.join(str(tmp_path), "test_paths")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_paths.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    for name in ("junctions", "ring4"):
        pts, table, _, joins = _cases()[name]
        words = [len(table)]
        for s, n, fl, _ in table.tolist():
            words += [n, fl] + pts[s:s + n].reshape(-1).tolist()
        partners = np.where(joins[:, 4] & JM.MUTUAL, joins[:, 3], -1).astype(np.int32)
        src, mid, dst = (os.path.join(str(tmp_path), "%s.%s" % (name, n)) for n in ("chains", "partners", "paths"))
        np.array(words, np.int32).tofile(src)
        partners.tofile(mid)
        r = subprocess.run([exe, src, mid, dst], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        want = _want(name)
        assert "paths OK (%d chains, %d paths)" % (len(table), want["counts"][0]) in r.stdout, r.stdout
        got = np.fromfile(dst, np.int32).tolist()
        expect = [want["counts"][0]]
        for p, (start, length, flags, _) in enumerate(want["paths"].tolist()):
            i = want["info"][p]
            mem = want["members"][i["first_member"]:i["first_member"] + i["n_members"]]
            expect += [flags, len(mem)] + [2 * int(x["chain"]) + int(x["flags"] & M.MEMBER_REVERSED) for x in mem]
            expect += [length] + want["path_points"][start:start + length].reshape(-1).tolist()
        assert got == expect, name
