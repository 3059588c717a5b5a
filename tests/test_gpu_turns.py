"""GPU test (-m gpu): contour turns -- cvs_chain_turns, chain_turns / contour_corners and the facade's cornerContours against the model of
turns_model.py.

Every field of every record is held BIT FOR BIT: all arithmetic of a point is sequential in one lane, in the order the contract names, so
there is no tolerance anywhere; the summary is integers and a minimum with a first-index tie rule.  Two calls, the device and the host
path, and a captured graph give the same bytes."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import chains_batch_model as CBM
import chains_model as CM
import cvsteer_amd as cv
import refine_model as RM
import turns_model as M
from cvsteer_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32 = np.float32
GUARD = 64
SENTINEL = 0x5A5A5A5A
# (radius, min_arm, nms): the defaults, no suppression, the smallest and the largest radius, min_arm < radius, the widest window
CONFIGS = ((5, 5, 5), (5, 5, 0), (1, 1, 5), (64, 64, 5), (5, 2, 5), (7, 3, 64))
_cache = {}


def _filters(shape=(33, 65)):
    if shape not in _cache:
        _cache[shape] = cv.SteerableFiltersG2(torch.zeros(shape, device=DEV))
    return _cache[shape]


def _up(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _walk(n, seed):
    """n points of a king's walk: every step goes to an 8-neighbour, some of them back on the step before"""
    rng = np.random.default_rng(seed)
    steps = np.array([(1, 0), (1, 1), (0, 1), (1, -1), (-1, 1), (0, -1)])[rng.integers(0, 6, max(n - 1, 0))]
    return np.concatenate([[[300, 500]], [300, 500] + np.cumsum(steps, axis=0)]).astype(np.int32) if n > 1 else np.int32([[300, 500]])


def _hand_made():
    """open chains of 1, 2, 3, 10, 11, 12, 64, 65, 256, 257 and 1000 points, closed chains of 3, 4, 10, 11, 12 and 300 points and an isolated
    point, laid out so that chains straddle lane 63 / 64 and element 255 / 256 (and 511 / 512, ...) of the point list"""
    layout = [(10, 0), (12, 0), (11, 0), (3, 0), (2, 0), (1, 0), (3, 1), (4, 1), (10, 1), (11, 1), (12, 1), (64, 0), (65, 0), (300, 1), (256, 0),
              (257, 0), (1, 0), (1000, 0)]
    lists = [_walk(n, 7 + k) for k, (n, _) in enumerate(layout)]
    points, chains = M.pack(lists, [cl for _, cl in layout])
    inside = lambda e: any(s < e < s + n for s, n in chains[:, :2].tolist())       # elements e - 1 and e lie in one chain
    assert inside(64) and inside(256) and inside(512) and inside(1024)
    assert chains[9].tolist() == [56, 11, 1, 0] and chains[13].tolist() == [208, 300, 1, 0]
    return points, chains


@functools.lru_cache(maxsize=None)
def _cases():
    cases = {"hand made": _hand_made()}
    for density in (0.15, 0.5):
        mask = (np.random.default_rng(int(100 * density)).random((33, 65)) < density).astype(F32)
        cases["random %.2f" % density] = CM.chains(mask)
    masks = [(np.random.default_rng(40 + z).random((20, 31)) < 0.3).astype(F32) for z in range(3)]
    pts, chains, _ = CBM.chains_batch(masks)                                    # global starts, the plane in `reserved`
    assert chains[:, 3].max() == 2
    cases["batch"] = (pts, chains)
    out = {}
    for name, (pts, chains) in cases.items():
        rng = np.random.default_rng(len(pts))
        xy = (pts + rng.uniform(-0.5, 0.5, pts.shape)).astype(F32)
        arrays = tuple(np.ascontiguousarray(a) for a in (np.asarray(pts, np.int32), np.asarray(chains, np.int32), xy))
        for a in arrays:
            a.setflags(write=False)
        out[name] = arrays
    return out


@functools.lru_cache(maxsize=None)
def _want(name, with_xy, cfg):
    pts, chains, xy = _cases()[name]
    radius, min_arm, nms = cfg
    return M.turns(pts, chains, xy if with_xy else None, radius=radius, min_arm=min_arm, nms=nms, summary=True)


def _call(f, name, with_xy, cfg, path, summary=True, chains=None):
    pts, table, xy = _cases()[name]
    put = _up if path == "device" else (lambda a: None if a is None else np.array(a))
    radius, min_arm, nms = cfg
    return f.chain_turns(put(pts), put(table if chains is None else chains), xy=put(xy if with_xy else None), radius=radius, min_arm=min_arm,
                         nms=nms, summary=summary)


@pytest.mark.parametrize("name", ["hand made", "random 0.15", "random 0.50", "batch"])
def test_turns_bit_for_bit(name):
    f = _filters()
    seen = 0
    for cfg in CONFIGS:
        for with_xy in (False, True):
            want, want_sum = _want(name, with_xy, cfg)
            got, got_sum = _call(f, name, with_xy, cfg, "device")
            assert got.dtype == M.TURN_DTYPE and got_sum.dtype == M.SUMMARY_DTYPE
            for field in M.TURN_DTYPE.names:                                      # field by field first: a failure names it
                assert got[field].tobytes() == want[field].tobytes(), (cfg, with_xy, field, np.nonzero(got[field].view(np.int32) != want[field].view(np.int32))[0][:8])
            assert M.same_records(got, want) and M.same_records(got_sum, want_sum), (cfg, with_xy)
            assert M.same_records(_call(f, name, with_xy, cfg, "device", summary=False), want)     # two launches: the same table
            seen |= int(np.bitwise_or.reduce(want["flags"]))
    assert seen & M.CORNER and seen & M.END and seen & M.SHORT and not seen & M.NO_CHAIN
    cfg = CONFIGS[0]
    for with_xy in (False, True):
        a, sa = _call(f, name, with_xy, cfg, "device")
        b, sb = _call(f, name, with_xy, cfg, "host")
        want, want_sum = _want(name, with_xy, cfg)
        assert M.same_records(a, want) and M.same_records(b, want) and M.same_records(sa, want_sum) and M.same_records(sb, want_sum)
        assert M.same_records(_call(f, name, with_xy, cfg, "host", summary=False), want)
    if name == "hand made":
        want, want_sum = _want(name, False, CONFIGS[0])
        assert (want_sum["corners"] > 0).sum() >= 4 and (want_sum["eligible"] == 0).sum() >= 6 and (want_sum["sharpest"] == -1).sum() >= 6
        assert (_want(name, False, (64, 64, 5))[0]["nb"] == 64).any()
    if name == "batch":
        assert _cases()[name][1][:, 3].any() and _want(name, False, CONFIGS[0])[0]["chain"].max() == len(_cases()[name][1]) - 1


def test_plateau_keeps_the_first():
    pts = np.int32([(0, 0), (1, 0), (2, 0), (3, 1), (4, 1), (5, 1)])              # symmetric under a half turn: cos[2] == cos[3]
    tab = np.int32([[0, 6, 0, 0]])
    f = _filters()
    got = f.chain_turns(_up(pts), _up(tab), radius=2, min_arm=2, nms=2, max_cos=1.0)
    assert got["cos"][2] == got["cos"][3] and (got["flags"][2], got["flags"][3]) == (M.CORNER, 0)
    assert M.same_records(got, M.turns(pts, tab, radius=2, min_arm=2, nms=2, max_cos=1.0))
    none = f.chain_turns(_up(pts), _up(tab), radius=2, min_arm=2, nms=0, max_cos=1.0)
    assert (none["flags"][2:4] == M.CORNER).all() and M.same_records(none, M.turns(pts, tab, radius=2, min_arm=2, nms=0, max_cos=1.0))
    # the same on a closed chain, where the window wraps: a square ring has four equal corners; nms = 1 keeps them all, and once the window
    # reaches the next corner each has an equal one BEHIND it -- a cycle of equal minima has no first, and the strict comparison drops all
    ring = np.int32([(0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (1, 2), (0, 2), (0, 1)])
    rtab = np.int32([[0, 8, M.CLOSED, 0]])
    for nms in (1, 2, 64):
        got = f.chain_turns(_up(ring), _up(rtab), radius=1, min_arm=1, nms=nms, max_cos=0.5)
        assert M.same_records(got, M.turns(ring, rtab, radius=1, min_arm=1, nms=nms, max_cos=0.5)), nms
        assert np.nonzero(got["flags"] & M.CORNER)[0].tolist() == ([0, 2, 4, 6] if nms == 1 else []), nms


def test_nan_in_xy_marks_its_windows():
    pts, chains, xy = _cases()["hand made"]
    xy = np.array(xy)
    hit = [100, 300, 1500]                                                      # inside the open 64, the closed 300 and the open 1000
    xy[hit, 0] = np.nan
    f = _filters()
    got = f.chain_turns(_up(pts), _up(chains), xy=_up(xy), radius=5)
    want = M.turns(pts, chains, xy, radius=5)
    assert M.same_records(got, want)
    clean = _want("hand made", True, (5, 5, 5))[0]
    marked = np.nonzero((got["flags"] & M.DEGENERATE) & ~(clean["flags"] & M.DEGENERATE))[0].tolist()
    assert marked == [i for h in hit for i in range(h - 5, h + 6)]              # exactly the points whose window holds it
    assert np.isnan(got["cos"][marked]).all() and not (got["flags"][marked] & M.CORNER).any()


# ---- capture ----
def test_graph_capture():
    pts, chains, xy = (_up(a) for a in _cases()["random 0.15"])
    f = cv.SteerableFiltersG2(torch.zeros((33, 65), device=DEV))
    want, want_sum = _want("random 0.15", True, (5, 5, 5))
    tab = torch.empty((len(pts), 32), dtype=torch.uint8, device=DEV)
    sums = torch.empty((len(chains), 16), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f.chain_turns(pts, chains, xy=xy, summary=True, out=(tab, sums))        # the handle moves to the side stream outside the capture
        torch.cuda.synchronize()
        tab.fill_(7), sums.fill_(7)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            assert f.chain_turns(pts, chains, xy=xy, summary=True, out=(tab, sums))[0] is tab
            hp, hc = np.int32([[0, 0], [1, 0]]), np.int32([[0, 2, 0, 0]])       # host arrays are refused while capturing
            ht = np.full((2, 8), -9, np.int32)
            cfg = L.TurnCfg(5, 5, 5, 0.5)
            p = lambda a: C.c_void_p(a.ctypes.data)
            rc = L.lib().cvs_chain_turns(f._h, p(hp), 2, p(hc), 1, None, C.byref(cfg), p(ht), None, L.MEM_HOST)
    assert rc == L.E_UNSUPPORTED and (ht == -9).all()
    torch.cuda.synchronize()
    assert bool((tab == 7).all()) and bool((sums == 7).all())                   # a capture runs nothing
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert tab.cpu().numpy().view(M.TURN_DTYPE).reshape(-1).tobytes() == want.tobytes()
        assert sums.cpu().numpy().view(M.SUMMARY_DTYPE).reshape(-1).tobytes() == want_sum.tobytes()
        tab.fill_(7), sums.fill_(7)
    assert f.chain_turns(hp, hc)["flags"].tolist() == [M.END | M.SHORT] * 2     # the handle works on, on both paths
    assert M.same_records(f.chain_turns(pts, chains, xy=xy), want)


# ---- raw calls: guarded arrays, broken tables, errors ----
def _guarded(n, words):
    """(buffer, view): n records of `words` int32 words with GUARD records of sentinel in front and behind"""
    buf = torch.full((GUARD + n + GUARD, words), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _ptr(a):
    return None if a is None else C.c_void_p(a if isinstance(a, int) else (a.data_ptr() if torch.is_tensor(a) else a.ctypes.data))


def _raw(f, pts, n, chains, m, xy, cfg, table, summary, mem):
    cfg = None if cfg is None else C.byref(L.TurnCfg(*cfg))
    return L.lib().cvs_chain_turns(f._h, _ptr(pts), n, _ptr(chains), m, _ptr(xy), cfg, _ptr(table), _ptr(summary), mem)


def test_broken_device_tables_give_no_chain_and_write_nothing_outside():
    pts, chains, xy = _cases()["hand made"]
    n, m = len(pts), len(chains)
    f = _filters()
    dp, dx = _up(pts), _up(xy)
    f._bind_stream(dp)
    gap, long_, negative, beyond, shuffled = (np.array(chains) for _ in range(5))
    gap[11, 1] = 30                                                             # the open 64 keeps 30 points: a gap of 34 behind it
    long_[-1, 1] += 1                                                           # the last chain leaves the array
    negative[5, 1] = -3                                                         # a negative length
    beyond[-2:, 0] += n                                                         # starts no point reaches: the search ends in front of them
    shuffled[:, 0] = shuffled[::-1, 0]                                          # starts that descend: which entry the search finds is unspecified
    shuffled[3, 0], shuffled[7, 0] = -2 ** 31, 2 ** 31 - 1
    for what, tab, sorted_ in (("a gap", gap, True), ("a chain that leaves the array", long_, True), ("a negative length", negative, True),
                               ("starts beyond the points", beyond, True), ("descending starts", shuffled, False)):
        tbuf, tview = _guarded(n, 8)
        sbuf, sview = _guarded(m, 4)
        inputs = [torch.cat([torch.full((GUARD,) + a.shape[1:], 77, dtype=a.dtype, device=DEV), a, torch.full((GUARD,) + a.shape[1:], 77, dtype=a.dtype, device=DEV)])
                  for a in (dp, _up(tab), dx)]
        before = [a.clone() for a in inputs]
        gp, gc, gx = (a[GUARD:len(a) - GUARD] for a in inputs)
        assert _raw(f, gp, n, gc, m, gx, (5, 5, 5, M.COS45), tview, sview, L.MEM_DEVICE) == 0, what
        torch.cuda.synchronize()
        assert _guards_intact(tbuf, n) and _guards_intact(sbuf, m), what
        assert all(torch.equal(a, b) for a, b in zip(inputs, before)), what     # no input is written
        got = tview.cpu().numpy().view(M.TURN_DTYPE).reshape(-1)
        got_sum = sview.cpu().numpy().view(M.SUMMARY_DTYPE).reshape(-1)
        none = got["chain"] == -1
        assert ((got["flags"] & M.NO_CHAIN) != 0).tolist() == none.tolist(), what
        blank = np.zeros(1, M.TURN_DTYPE)
        blank["chain"], blank["flags"] = -1, M.NO_CHAIN
        blank["sin"] = blank["cos"] = np.uint32(M.QNAN_BITS).view(F32)
        assert all(r.tobytes() == blank.tobytes() for r in got[none]), what     # chain -1, NO_CHAIN, zeros, NaN in sin and cos
        c = got["chain"][~none].astype(np.int64)
        i = np.nonzero(~none)[0]
        assert (c >= 0).all() and (c < m).all() and (tab[c, 0] <= i).all() and (i < tab[c, 0].astype(np.int64) + tab[c, 1]).all(), what
        if sorted_:
            want, want_sum = M.turns(pts, tab, xy, summary=True)
            assert none.any() and M.same_records(got, want) and M.same_records(got_sum, want_sum), what
        # the same table on the host is refused, and the outputs are untouched
        ht, hs = np.full((n, 8), -9, np.int32), np.full((m, 4), -9, np.int32)
        keep = [np.array(pts), np.ascontiguousarray(tab), np.array(xy)]
        assert _raw(f, keep[0], n, keep[1], m, keep[2], (5, 5, 5, M.COS45), ht, hs, L.MEM_HOST) == L.E_BADARG, what
        assert (ht == -9).all() and (hs == -9).all(), what
        with pytest.raises(cv.CvsError) as ei:
            f.chain_turns(keep[0], keep[1], xy=keep[2])
        assert ei.value.status == L.E_BADARG


def test_errors_leave_the_outputs_untouched():
    pts, chains, xy = _cases()["random 0.15"]
    f = _filters()
    dp, dc, dx = (_up(a) for a in (pts, chains, xy))
    n, m, D, H, B = len(pts), len(chains), L.MEM_DEVICE, L.MEM_HOST, L.E_BADARG
    ok = (5, 5, 5, 0.5)
    tab = torch.full((n + 1, 8), -9, dtype=torch.int32, device=DEV)
    sums = torch.full((m, 4), -9, dtype=torch.int32, device=DEV)
    f._bind_stream(dp)
    call = lambda p, n_, c, m_, x, cfg, t, s, mem: _raw(f, p, n_, c, m_, x, cfg, t, s, mem)
    # nothing to do: CVS_OK, nothing queued, nothing written
    assert call(dp, 0, dc, m, dx, ok, tab, sums, D) == 0 and call(None, 0, None, 0, None, ok, None, None, D) == 0
    assert call(None, 0, None, 0, None, ok, None, None, H) == 0
    # cfg
    assert call(dp, n, dc, m, dx, None, tab, sums, D) == B
    for bad in ((0, 1, 0, 0.5), (65, 5, 5, 0.5), (-1, 1, 1, 0.5), (5, 0, 5, 0.5), (5, 6, 5, 0.5), (5, 5, -1, 0.5), (5, 5, 65, 0.5),
                (5, 5, 5, float("nan")), (5, 5, 5, 1.5), (5, 5, 5, -1.5), (5, 5, 5, float("inf"))):
        assert call(dp, n, dc, m, dx, bad, tab, sums, D) == B, bad
    # counts, arrays, mem
    assert call(dp, -1, dc, m, dx, ok, tab, sums, D) == B and call(dp, n, dc, -1, dx, ok, tab, sums, D) == B
    assert call(None, n, dc, m, dx, ok, tab, sums, D) == B and call(dp, n, None, m, dx, ok, tab, sums, D) == B
    assert call(dp, n, dc, m, dx, ok, None, sums, D) == B and call(dp, n, None, 0, dx, ok, tab, None, D) == B   # points without a chain
    assert call(dp, n, dc, m, dx, ok, tab, sums, 5) == B and call(dp, n, dc, m, dx, ok, tab, sums, -1) == B
    for k in range(5):                                                          # not aligned to 4 bytes
        args = [dp, dc, dx, tab, sums]
        args[k] = args[k].data_ptr() + 2
        assert call(args[0], n, args[1], m, args[2], ok, args[3], args[4], D) == B, k
    for a in (dp, dc, dx):                                                      # an output over an input, and over the other output
        assert call(dp, n, dc, m, dx, ok, a, sums, D) == B and call(dp, n, dc, m, dx, ok, tab, a, D) == B
    assert call(dp, n, dc, m, dx, ok, tab, tab, D) == B and call(dp, n, dc, m, dx, ok, tab, tab.data_ptr() + 32 * (n - 1), D) == B
    assert call(dp, 2 ** 30 + 1, dc, m, None, ok, tab, None, D) == L.E_SIZE
    # host tables that do not say what the contract says
    ht, hs = np.full((n, 8), -9, np.int32), np.full((m, 4), -9, np.int32)
    host = lambda c, m_=m: call(np.array(pts), n, np.ascontiguousarray(c), m_, np.array(xy), ok, ht, hs, H)
    for row, col, delta in ((-1, 1, 1), (-1, 1, -1), (0, 0, -1), (0, 0, 1), (1, 0, 1), (m // 2, 1, -int(chains[m // 2, 1]))):
        bad = np.array(chains)
        bad[row, col] += delta
        assert host(bad) == B, (row, col, delta)
    assert host(chains[:-1], m - 1) == B                                        # lengths that stop short of n_points
    torch.cuda.synchronize()
    assert bool((tab == -9).all()) and bool((sums == -9).all()) and (ht == -9).all() and (hs == -9).all()
    # the same arrays unharmed: the calls go through, also into a table that is aligned to 4 bytes only
    want, want_sum = M.turns(pts, chains, xy, max_cos=0.5, summary=True)
    assert host(chains) == 0 and ht.view(M.TURN_DTYPE).reshape(-1).tobytes() == want.tobytes()
    assert hs.view(M.SUMMARY_DTYPE).reshape(-1).tobytes() == want_sum.tobytes()
    flat = tab.reshape(-1)
    assert call(dp, n, dc, m, dx, ok, flat.data_ptr() + 4, sums.data_ptr(), D) == 0
    torch.cuda.synchronize()
    assert flat[1:1 + 8 * n].cpu().numpy().view(M.TURN_DTYPE).tobytes() == want.tobytes() and int(flat[0]) == -9 and bool((flat[1 + 8 * n:] == -9).all())
    assert sums.cpu().numpy().view(M.SUMMARY_DTYPE).reshape(-1).tobytes() == want_sum.tobytes()


# ---- end to end ----
def test_chain_turns_and_contour_corners_on_the_l_ridge():
    img, theta, (vx, vy), mask = M.ridge_case(0.0, 90.0)
    f = cv.SteerableFiltersG2(_up(img))
    d_img, d_theta, d_mask = _up(img), _up(theta), _up(mask)
    pts, chains = CM.chains(mask)
    xy, _ = RM.refine(pts, img, theta)
    want = M.turns(pts, chains, xy)
    corner_xy, corner_index, turns, table = f.contour_corners(d_mask, d_img, theta=d_theta)
    assert np.array_equal(table.cpu().numpy(), chains) and M.same_records(turns, want)
    assert corner_index.tolist() == np.nonzero(want["flags"] & M.CORNER)[0].tolist() and len(corner_index) == 1
    assert corner_xy.dtype == F32 and corner_xy.tobytes() == xy[corner_index].tobytes()
    assert float(np.hypot(corner_xy[0, 0] - vx, corner_xy[0, 1] - vy)) <= 1.0
    # its own three-call composition, the integer points, the configuration, and the numpy path
    d_pts, d_chains = f.contour_chains(d_mask)
    d_xy, _ = f.chain_refine(d_pts, d_img, d_theta)
    assert M.same_records(f.chain_turns(d_pts, d_chains, xy=d_xy), want)
    assert M.same_records(f.chain_turns(d_pts, d_chains), M.turns(pts, chains))
    cfg = dict(radius=3, min_arm=2, nms=1, max_cos=0.9)
    got = f.contour_corners(d_mask, d_img, theta=d_theta, **cfg)
    assert M.same_records(got[2], M.turns(pts, chains, xy, **cfg)) and len(got[1]) >= 1
    host = f.contour_corners(mask, img, theta=theta)
    assert M.same_records(host[2], want) and host[0].tobytes() == corner_xy.tobytes() and host[1].tolist() == corner_index.tolist()
    # out=: the tables stay on the device
    tab = torch.empty((len(pts), 32), dtype=torch.uint8, device=DEV)
    assert f.chain_turns(d_pts, d_chains, xy=d_xy, out=tab) is tab
    assert tab.cpu().numpy().view(M.TURN_DTYPE).reshape(-1).tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        f.chain_turns(d_pts, d_chains, xy=d_xy, out=tab[:-1])


# ---- facade ----
def test_facade_member(tmp_path):
    exe = os.path.join(str(tmp_path), "test_turns")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_turns.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    img, _, _, mask = M.ridge_case(0.0, 90.0)
    pts, table = CM.chains(mask)
    words = [len(table)]
    for s, n, fl, _ in table.tolist():
        words += [n, fl] + pts[s:s + n].reshape(-1).tolist()
    src_img, src, dst = (os.path.join(str(tmp_path), n) for n in ("image.f32", "chains.i32", "corners.f32"))
    np.ascontiguousarray(img, F32).tofile(src_img)
    np.array(words, np.int32).tofile(src)
    r = subprocess.run([exe, src_img, "48", "48", src, "5", "0.70710678", dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dst, F32).reshape(-1, 3)                                  # chain, offset, cos
    f = cv.SteerableFiltersG2(img)                                              # the facade's defaults: the same engine, its own theta
    xy, _ = f.chain_refine(pts, img)
    turns = f.chain_turns(pts, table, xy=xy, radius=5, max_cos=0.70710678)
    at = np.nonzero(turns["flags"] & M.CORNER)[0]
    assert "turns OK (%d chains, %d corners)" % (len(table), len(at)) in r.stdout, r.stdout
    assert len(got) == len(at) >= 1
    assert got[:, 0].tolist() == turns["chain"][at].tolist() and got[:, 1].tolist() == (at - table[turns["chain"][at], 0]).tolist()
    assert got[:, 2].tobytes() == turns["cos"][at].tobytes()
