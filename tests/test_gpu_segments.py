"""GPU test (-m gpu): contour segments -- cvs_polyline_segments, polyline_segments / contour_segments and the facade's fitSegments against
the model of segments_model.py.

first, count, chain and flags are the model's exactly.  Each of the six sums lies within (count + 2) 2^-52 sum|term| of the exact sum: a
term carries at most two roundings of 2^-53 and any order of n additions adds at most (n - 1) 2^-53 sum|term|, so the bound holds for every
order with a factor of two to spare -- nothing in it is measured.  The eight derived fields are held BIT FOR BIT to the model's derived
sequence applied to the record's own stored sums.  Two calls, and the device and the host path, give the same bytes."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import chains_batch_model as CBM
import chains_model as CM
import contour_model as NM
import cvsteer_amd as cv
import polyline_model as PM
import refine_model as RM
import segments_model as M
from cvsteer_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32 = np.float32
COMBOS = ((True, True), (False, False), (True, False), (False, True))         # (xy, strength) present or absent
_cache = {}


def _filters(shape=(33, 65)):
    if shape not in _cache:
        _cache[shape] = cv.SteerableFiltersG2(torch.zeros(shape, device=DEV))
    return _cache[shape]


def _up(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _walk(n, seed):
    """n points of a king's walk: every step goes to an 8-neighbour"""
    rng = np.random.default_rng(seed)
    steps = np.array([(1, 0), (1, 1), (0, 1), (1, -1)])[rng.integers(0, 4, max(n - 1, 0))]
    return np.concatenate([[[3, 500]], [3, 500] + np.cumsum(steps, axis=0)]).astype(np.int32) if n > 1 else np.int32([[3, 500]])


def _hand_made():
    """(points, chains, polylines, index) placed by hand: one open walk whose spans have 2, 3, 16, 17, 64, 65, 256, 257 and 1000 points
    (both sides of the 16-lane group, of a wave's 64 lanes and of the group / workgroup boundary), a closed ring with three vertices (its
    last span wraps, in a lane group), a closed cycle of 300 points with one vertex (301 points that wrap, in a workgroup), an isolated
    point and an open chain of two points"""
    counts = (2, 3, 16, 17, 64, 65, 256, 257, 1000)
    marks = np.concatenate([[0], np.cumsum(np.array(counts) - 1)])           # a vertex belongs to both of its spans
    ring = [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (3, 2), (3, 3), (2, 3), (1, 3), (0, 3), (0, 2), (0, 1)]
    lists = [_walk(int(marks[-1]) + 1, 1), np.int32(ring), _walk(300, 9), np.int32([[7, 7]]), np.int32([[4, 4], [5, 5]])]
    flags = [0, CM.CLOSED, CM.CLOSED, 0, 0]
    local = [marks.tolist(), [1, 4, 9], [17], [0], [0, 1]]
    points = np.concatenate(lists).astype(np.int32).reshape(-1, 2)
    chains, polylines, index, start = [], [], [], 0
    for p, fl, idx in zip(lists, flags, local):
        chains.append((start, len(p), fl, 0))
        polylines.append((len(index), len(idx), fl, 0))
        index += [start + i for i in idx]
        start += len(p)
    return points, np.int32(chains), np.int32(polylines), np.int32(index)


@functools.lru_cache(maxsize=None)
def _cases():
    cases = {"hand made": _hand_made()}
    for density in (0.15, 0.5):
        mask = (np.random.default_rng(int(100 * density)).random((33, 65)) < density).astype(F32)
        pts, chains = CM.chains(mask)
        cases["random %.2f" % density] = (pts, chains) + PM.polylines(pts, chains, 1.0)[1:]
    masks = [(np.random.default_rng(40 + z).random((20, 31)) < 0.3).astype(F32) for z in range(3)]
    pts, chains, _ = CBM.chains_batch(masks)                                  # global starts, the plane in `reserved`
    assert chains[:, 3].max() == 2
    cases["batch"] = (pts, chains) + PM.polylines(pts, chains, 1.0)[1:]
    out = {}
    for name, (pts, chains, pol, idx) in cases.items():
        rng = np.random.default_rng(len(pts))
        xy = (pts + rng.uniform(-0.5, 0.5, pts.shape)).astype(F32)
        strength = rng.standard_normal(len(pts)).astype(F32)
        strength[rng.random(len(pts)) < 0.03] = np.nan
        arrays = tuple(np.ascontiguousarray(a) for a in (pts, chains, pol, idx, xy, strength))
        for a in arrays:
            a.setflags(write=False)
        out[name] = arrays
    return out


@functools.lru_cache(maxsize=None)
def _want(name, with_xy, with_strength):
    pts, chains, pol, idx, xy, strength = _cases()[name]
    return M.segments(pts, chains, pol, idx, xy if with_xy else None, strength if with_strength else None, return_abs=True)


def _call(f, name, with_xy, with_strength, path, tables=None):
    pts, chains, pol, idx, xy, strength = _cases()[name]
    chains, pol, idx = tables or (chains, pol, idx)
    put = _up if path == "device" else (lambda a: None if a is None else np.array(a))
    return f.polyline_segments(put(pts), put(chains), put(pol), put(idx), xy=put(xy if with_xy else None),
                               strength=put(strength if with_strength else None))


def _same_doubles(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def _check(got, name, with_xy, with_strength):
    pts, chains, pol, idx, xy, strength = _cases()[name]
    want, mags = _want(name, with_xy, with_strength)
    assert isinstance(got, np.ndarray) and got.dtype == M.SEGMENT_DTYPE and got.shape == (len(idx),)
    for field in ("first", "count", "chain", "flags"):
        assert np.array_equal(got[field], want[field]), field
    n = got["count"].astype(np.float64)
    for j, field in enumerate(M.SUMS):
        assert np.isfinite(got[field]).all()
        assert (np.abs(got[field] - want[field]) <= (n + 2) * 2.0 ** -52 * mags[:, j]).all(), field
    # the derived fields: the model's sequence on the record's OWN sums, bit for bit
    own = got.copy()
    sp = M.spans(chains, pol, idx, len(pts))
    for k, (_, count, _, flags, pos) in enumerate(sp):
        for field in M.DERIVED:
            own[k][field] = 0.0
        own[k]["flags"] = flags
        if pos is not None:
            M.finish(own[k], pts.astype(np.int64), xy if with_xy else None, pos)
    assert np.array_equal(own["flags"], got["flags"])
    for field in M.DERIVED:
        assert _same_doubles(got[field], own[field]), field
    empty = got["count"] == 0
    assert not got[empty].view(np.uint8).reshape(-1, 128)[:, 12:].any()         # no span: zeros behind `chain`
    return want


@pytest.mark.parametrize("name", ["hand made", "random 0.15", "random 0.50", "batch"])
def test_segments(name):
    f = _filters()
    for with_xy, with_strength in COMBOS:
        got = _call(f, name, with_xy, with_strength, "device")
        want = _check(got, name, with_xy, with_strength)
        assert _call(f, name, with_xy, with_strength, "device").tobytes() == got.tobytes()       # two calls: identical bytes
        assert _call(f, name, with_xy, with_strength, "host").tobytes() == got.tobytes()         # one pair of kernels behind both paths
    fitted = want[want["count"] >= 2]
    assert len(fitted) >= 8 and (want["count"] == 0).sum() >= 2
    if name == "hand made":
        assert want["count"].tolist() == [2, 3, 16, 17, 64, 65, 256, 257, 1000, 0, 4, 6, 5, 301, 0, 2, 0]
        assert (want["flags"] & M.WRAPS).tolist() == [0] * 12 + [M.WRAPS, M.WRAPS] + [0] * 3
    if name == "batch":
        assert _cases()[name][1][:, 3].any() and want["chain"].max() == len(_cases()[name][1]) - 1


def test_degenerate_spans_on_the_device():
    """all weights 0, all positions equal, and a NaN position: flagged, NaN in the line, the sums as they came out"""
    pts = np.int32([[0, 0], [1, 0], [2, 1], [3, 1], [4, 2], [5, 2]])
    chains, pol, idx = np.int32([[0, 6, 0, 0]]), np.int32([[0, 4, 0, 0]]), np.int32([0, 2, 4, 5])
    xy = F32([[0, 0], [1.25, 0], [2, 1], [np.nan, 1], [4, 2], [4, 2]])
    st = F32([-1, 0, np.nan, 1, 1, 1])
    f = _filters()
    got = f.polyline_segments(_up(pts), _up(chains), _up(pol), _up(idx), xy=_up(xy), strength=_up(st))
    want = M.segments(pts, chains, pol, idx, xy, st)
    assert want["flags"].tolist() == [M.DEGENERATE] * 3 + [0] and want["count"].tolist() == [3, 3, 2, 0]
    for field in M.SEGMENT_DTYPE.names:
        assert _same_doubles(got[field], want[field]) if field in M.SUMS + M.DERIVED else np.array_equal(got[field], want[field]), field
    assert got["w"][0] == 0 and np.isnan(got["cx"][0]) and np.isnan(got["sx"][1]) and got["cx"][2] == 4.0 and np.isnan(got["ux"]).sum() == 3
    assert f.polyline_segments(pts, chains, pol, idx, xy=xy, strength=st).tobytes() == got.tobytes()


# ---- bad entries of device tables ----
def test_bad_device_entries_give_the_record_without_a_span():
    pts, chains, pol, idx, xy, strength = _cases()["hand made"]
    f = _filters()
    clean = _call(f, "hand made", True, True, "device")
    no_length, leaves, decreasing = np.array(chains), np.array(idx), np.array(idx)
    no_length[1, 1] = 0                                                         # the ring: its vertices 10, 11, 12 lose their spans
    leaves[3] = int(chains[0, 1]) + 5                                           # vertex 3 of the walk points into the ring: spans 2 and 3
    decreasing[9] = idx[8] - 10                                                 # the walk's last vertex lies before the one in front: span 8
    for what, tables, hit in (("a chain of length 0", (no_length, pol, idx), [10, 11, 12]),
                              ("an index that leaves its chain", (chains, pol, leaves), [2, 3]),
                              ("a decreasing index pair", (chains, pol, decreasing), [8])):
        got = _call(f, "hand made", True, True, "device", tables)
        want = M.segments(pts, tables[0], tables[1], tables[2], xy, strength)
        gone = np.nonzero((want["count"] == 0) & (clean["count"] > 0))[0].tolist()
        assert gone == hit, (what, gone)
        for k in gone:                                                          # the record without a span
            assert got[k].tobytes() == np.array([(int(tables[2][k]), 0, int(clean["chain"][k]), 0) + (0.0,) * 14], M.SEGMENT_DTYPE).tobytes(), (what, k)
        rest = np.setdiff1d(np.arange(len(idx)), gone)
        if what == "a decreasing index pair":                                   # (vertex 9 never had a span; its `first` is what the index says)
            assert got[9].tobytes() == np.array([(int(decreasing[9]), 0, 0, 0) + (0.0,) * 14], M.SEGMENT_DTYPE).tobytes()
            rest = np.setdiff1d(rest, [9])
        assert got[rest].tobytes() == clean[rest].tobytes(), what              # every other record: the clean call's bytes
        # the same tables on the host are refused, and the output is untouched
        ht = np.full((len(idx), 32), -9, np.int32)
        p = lambda a: C.c_void_p(np.ascontiguousarray(a).ctypes.data)
        keep = [np.ascontiguousarray(a) for a in (pts,) + tuple(tables) + (xy, strength)]
        rc = L.lib().cvs_polyline_segments(f._h, p(keep[0]), len(pts), p(keep[1]), p(keep[2]), len(chains), p(keep[3]), len(idx), p(keep[4]),
                                           p(keep[5]), C.c_void_p(ht.ctypes.data), L.MEM_HOST)
        assert rc == L.E_BADARG and (ht == -9).all(), what
        with pytest.raises(cv.CvsError) as ei:
            _call(f, "hand made", True, True, "host", tables)
        assert ei.value.status == L.E_BADARG


# ---- errors ----
def test_errors_leave_the_table_untouched():
    pts, chains, pol, idx, xy, strength = _cases()["random 0.15"]
    f = _filters()
    dp, dc, dl, di, dx, ds = (_up(a) for a in (pts, chains, pol, idx, xy, strength))
    n, m, v, D, H = len(pts), len(chains), len(idx), L.MEM_DEVICE, L.MEM_HOST
    tab = torch.full((v, 32), -9, dtype=torch.int32, device=DEV)
    f._bind_stream(dp)
    ptr = lambda a: None if a is None else C.c_void_p(a if isinstance(a, int) else (a.data_ptr() if torch.is_tensor(a) else a.ctypes.data))
    call = lambda p, n_, c, l, m_, i, v_, x, s, t, mem: L.lib().cvs_polyline_segments(f._h, ptr(p), n_, ptr(c), ptr(l), m_, ptr(i), v_, ptr(x),
                                                                                      ptr(s), ptr(t), mem)
    assert call(dp, n, dc, dl, m, di, 0, dx, ds, tab, D) == 0 and call(None, 0, None, None, 0, None, 0, None, None, None, D) == 0
    assert call(None, 0, None, None, 0, None, 0, None, None, None, H) == 0
    B = L.E_BADARG
    assert call(dp, -1, dc, dl, m, di, v, dx, ds, tab, D) == B and call(dp, n, dc, dl, -1, di, v, dx, ds, tab, D) == B
    assert call(dp, n, dc, dl, m, di, -1, dx, ds, tab, D) == B
    assert call(None, n, dc, dl, m, di, v, dx, ds, tab, D) == B and call(dp, n, None, dl, m, di, v, dx, ds, tab, D) == B
    assert call(dp, n, dc, None, m, di, v, dx, ds, tab, D) == B and call(dp, n, dc, dl, m, None, v, dx, ds, tab, D) == B
    assert call(dp, n, dc, dl, m, di, v, dx, ds, None, D) == B and call(dp, n, dc, dl, m, di, v, dx, ds, tab, 5) == B
    assert call(dp, n, None, None, 0, di, v, dx, ds, tab, D) == B                                   # vertices without a polyline
    for k in range(6):                                                                              # not aligned to 4 bytes
        args = [dp, dc, dl, di, dx, ds]
        args[k] = args[k].data_ptr() + 2
        assert call(args[0], n, args[1], args[2], m, args[3], v, args[4], args[5], tab, D) == B, k
    assert call(dp, n, dc, dl, m, di, v, dx, ds, tab.data_ptr() + 4, D) == B                          # the table: 8 bytes
    assert call(dp, n, dc, dl, m, di, v, dx, ds, tab.data_ptr() + 2, D) == B
    for a in (dp, dc, dl, di, dx, ds):                                                              # the table over an input
        assert call(dp, n, dc, dl, m, di, v, dx, ds, a, D) == B
    assert call(dp, 2 ** 30 + 1, dc, dl, m, di, v, None, None, tab, D) == L.E_SIZE
    # host tables that do not say what the contract says
    ht = np.full((v, 32), -9, np.int32)
    host = lambda c, l, i: call(np.array(pts), n, np.ascontiguousarray(c), np.ascontiguousarray(l), m, np.ascontiguousarray(i), v,
                                np.array(xy), np.array(strength), ht, H)
    bad = np.array(chains)
    bad[-1, 1] += 1
    assert host(bad, pol, idx) == B
    bad = np.array(chains)
    bad[0, 0] = -1
    assert host(bad, pol, idx) == B
    bad = np.array(pol)
    bad[1, 0] += 1                                                              # a start that is not the running sum
    assert host(chains, bad, idx) == B
    bad = np.array(pol)
    bad[-1, 1] += 1                                                             # lengths that do not add up to n_vertices
    assert host(chains, bad, idx) == B
    bad = np.array(pol)
    bad[-1, 1] -= 1
    assert host(chains, bad, idx) == B
    first = int(np.nonzero(pol[:, 1] >= 2)[0][0])
    k = int(pol[first, 0])
    bad = np.array(idx)
    bad[k + 1] = bad[k]                                                         # not strictly increasing
    assert host(chains, pol, bad) == B
    bad = np.array(idx)
    bad[k] = chains[first, 0] - 1 if chains[first, 0] > 0 else chains[first, 0] + chains[first, 1]   # outside [S, S + L)
    assert host(chains, pol, bad) == B
    torch.cuda.synchronize()
    assert bool((tab == -9).all()) and (ht == -9).all()
    assert host(chains, pol, idx) == 0 and (ht[:, 1] >= 0).all()               # the same tables unharmed: the call goes through


# ---- capture ----
def test_graph_capture_with_chain_refine():
    from helpers import rand_image
    img = torch.from_numpy(rand_image(64, 200, seed=6)).to(DEV)
    f = cv.SteerableFiltersG2(img)
    edges = f.pipeline(img)[5]
    mask = f.hysteresis(f.nonmax(edges), 0.0, 0.0)
    pts, chains = f.contour_chains(mask)
    _, pol, idx = f.chain_polylines(pts, chains, 1.0, return_index=True)
    assert len(chains) > 10 and len(idx) > len(chains)
    want_xy, want_st = f.chain_refine(pts, edges)
    want = f.polyline_segments(pts, chains, pol, idx, xy=want_xy, strength=want_st)
    assert (want["count"] >= 2).sum() > 10
    xy, st = torch.empty_like(want_xy), torch.empty_like(want_st)
    tab = torch.empty((len(idx), 128), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f.chain_refine(pts, edges, out=(xy, st))               # the handle moves to the side stream outside the capture
        torch.cuda.synchronize()
        xy.fill_(7.0), st.fill_(7.0), tab.fill_(7)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            f.chain_refine(pts, edges, out=(xy, st))
            assert f.polyline_segments(pts, chains, pol, idx, xy=xy, strength=st, out=tab) is tab
            # host arrays are refused while capturing
            hp, hc, hl, hi = np.int32([[0, 0], [1, 0]]), np.int32([[0, 2, 0, 0]]), np.int32([[0, 2, 0, 0]]), np.int32([0, 1])
            ht = np.full((2, 32), -9, np.int32)
            p = lambda a: C.c_void_p(a.ctypes.data)
            rc = L.lib().cvs_polyline_segments(f._h, p(hp), 2, p(hc), p(hl), 1, p(hi), 2, None, None, p(ht), L.MEM_HOST)
    assert rc == L.E_UNSUPPORTED and (ht == -9).all()
    torch.cuda.synchronize()
    assert bool((tab == 7).all())                                               # a capture runs nothing
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(xy, want_xy) and torch.equal(st, want_st)
        assert tab.cpu().numpy().view(M.SEGMENT_DTYPE).reshape(-1).tobytes() == want.tobytes()
        tab.fill_(7)
    # the handle works on, on both paths
    assert f.polyline_segments(hp, hc, hl, hi)["count"].tolist() == [2, 0]
    assert f.polyline_segments(pts, chains, pol, idx, xy=want_xy, strength=want_st).tobytes() == want.tobytes()


# ---- end to end ----
def _ridge_case(deg):
    img, theta, dist = RM.ridge(48, deg)
    c, s = RM.directions(theta)
    sel = NM.nonmax_parts(img, c, s)[0] > 0.5
    sel[:6], sel[-6:], sel[:, :6], sel[:, -6:] = False, False, False, False
    return img, theta, dist, sel.astype(F32)


def _angle_error(ux, uy, deg):
    return np.abs((np.rad2deg(np.arctan2(uy, ux)) - deg + 90.0) % 180.0 - 90.0)


@pytest.mark.parametrize("deg", [0.0, 37.0, 133.0])
def test_contour_segments_on_ridges(deg):
    img, theta, dist, mask = _ridge_case(deg)
    f = cv.SteerableFiltersG2(_up(img))
    d_img, d_theta, d_mask = _up(img), _up(theta), _up(mask)
    seg, lines = f.contour_segments(d_mask, d_img, 1.0, theta=d_theta)
    # its own four-call composition, byte for byte
    pts, chains = f.contour_chains(d_mask)
    _, pol, idx = f.chain_polylines(pts, chains, 1.0, return_index=True)
    xy, st = f.chain_refine(pts, d_img, d_theta)
    table = f.polyline_segments(pts, chains, pol, idx, xy=xy)
    keep = (table["count"] >= 2) & ((table["flags"] & M.DEGENERATE) == 0)
    assert seg.tobytes() == table[keep].tobytes() and lines.dtype == np.float64 and lines.shape == (len(seg), 4)
    assert lines.tobytes() == M.end_points(table[keep]).tobytes()
    weighted = f.contour_segments(d_mask, d_img, 1.0, theta=d_theta, weighted=True, min_points=8)[0]
    want = f.polyline_segments(pts, chains, pol, idx, xy=xy, strength=st)
    assert weighted.tobytes() == want[(want["count"] >= 8) & ((want["flags"] & M.DEGENERATE) == 0)].tobytes()
    # the straight segments: the bars of the geometry table
    long = seg[seg["count"] >= 8]
    assert len(long) >= 1
    ang = float(_angle_error(long["ux"], long["uy"], deg).max())
    off = float(np.abs(dist(long["cx"], long["cy"])).max())
    ends = float(np.abs(dist(lines[seg["count"] >= 8][:, [0, 2]], lines[seg["count"] >= 8][:, [1, 3]])).max())
    print("ridge %5.1f deg: %d spans of >= 8 points, angle error %.4f deg, anchor %.4f px and end points %.4f px from the true line"
          % (deg, len(long), ang, off, ends))
    assert ang <= 0.2 and off <= 0.03
    # the numpy path gives the same records
    hseg, hlines = f.contour_segments(mask, img, 1.0, theta=theta)
    assert hseg.tobytes() == seg.tobytes() and hlines.tobytes() == lines.tobytes()


# ---- facade ----
def test_facade_member(tmp_path):
    exe = os.path.join(str(tmp_path), "test_segments")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_segments.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    img, _, _, mask = _ridge_case(37.0)
    pts, table = CM.chains(mask)
    words = [len(table)]
    for s, n, fl, _ in table.tolist():
        words += [n, fl] + pts[s:s + n].reshape(-1).tolist()
    src_img, src, dst = (os.path.join(str(tmp_path), n) for n in ("image.f32", "chains.i32", "segments.f32"))
    np.ascontiguousarray(img, F32).tofile(src_img)
    np.array(words, np.int32).tofile(src)
    r = subprocess.run([exe, src_img, "48", "48", src, "1.0", dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dst, F32).reshape(-1, 6)                                  # chain, x0, y0, x1, y1, rms
    f = cv.SteerableFiltersG2(img)                                              # the facade's defaults: the same engine, its own theta
    _, pol, idx = f.chain_polylines(pts, table, 1.0, return_index=True)
    xy, _ = f.chain_refine(pts, img)
    seg = f.polyline_segments(pts, table, pol, idx, xy=xy)
    seg = seg[(seg["count"] >= 2) & ((seg["flags"] & M.DEGENERATE) == 0)]
    assert "segments OK (%d chains, %d segments)" % (len(table), len(seg)) in r.stdout, r.stdout
    assert len(got) == len(seg) >= 1 and np.array_equal(got[:, 0], seg["chain"].astype(F32))
    assert float(np.abs(got[:, 1:5] - M.end_points(seg)).max()) <= 1e-4
    assert np.array_equal(got[:, 5], seg["rms"].astype(F32))
