"""GPU test (-m gpu): contour joins -- cvs_chain_joins, chain_joins / contour_joins and the facade's joinContours against the model of
joins_model.py.

Every field of every record is held BIT FOR BIT: the arithmetic of an arm is sequential in one lane, in the order the contract names, a
pair of ends is evaluated from its smaller end by both, and the grouping of the ends is integers -- so there is no tolerance anywhere.
Two calls, the device and the host path, and a captured graph give the same bytes."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import chains_model as CM
import cvsteer_amd as cv
import joins_model as M
import refine_model as RM
import turns_model as TM
from cvsteer_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32 = np.float32
GUARD = 64
SENTINEL = 0x5A5A5A5A
# (radius, min_arm, min_cos): radius 1, 8 and 64, min_arm 1 and 3 (held to the radius), min_cos -1 and 0.5
CONFIGS = tuple((radius, min(min_arm, radius), min_cos) for radius in (1, 8, 64) for min_arm in (1, 3) for min_cos in (-1.0, 0.5))
_cache = {}


def _filters(shape=(33, 65)):
    if shape not in _cache:
        _cache[shape] = cv.SteerableFiltersG2(torch.zeros(shape, device=DEV))
    return _cache[shape]


def _up(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _junction_mask():
    """a plus, a T and a diagonal X of 9 x 9 side by side on the 33 x 65 plane, a blank column between them"""
    mask = np.zeros((33, 65), F32)
    mask[6, 2:11], mask[2:11, 6] = 1, 1
    mask[14, 20:29], mask[14:23, 24] = 1, 1
    for k in range(9):
        mask[20 + k, 40 + k], mask[20 + k, 48 - k] = 1, 1
    return mask


def _jitter(pts):
    """the points plus a fixed sub-pixel jitter"""
    return (pts + np.random.default_rng(len(pts)).uniform(-0.4, 0.4, pts.shape)).astype(F32)


@functools.lru_cache(maxsize=None)
def _cases():
    cases = {"junctions": CM.chains(_junction_mask())}
    for density in (0.2, 0.5):
        mask = (np.random.default_rng(int(100 * density)).random((64, 64)) < density).astype(F32)
        cases["random %.2f" % density] = CM.chains(mask)
    out = {}
    for name, (pts, chains) in cases.items():
        arrays = tuple(np.ascontiguousarray(a) for a in (np.asarray(pts, np.int32), np.asarray(chains, np.int32), _jitter(pts)))
        for a in arrays:
            a.setflags(write=False)
        out[name] = arrays
    return out


@functools.lru_cache(maxsize=None)
def _want(name, with_xy, cfg):
    pts, chains, xy = _cases()[name]
    radius, min_arm, min_cos = cfg
    want = M.joins(pts, chains, xy if with_xy else None, radius=radius, min_arm=min_arm, min_cos=min_cos)
    want.setflags(write=False)
    return want


def _call(f, name, with_xy, cfg, path):
    pts, table, xy = _cases()[name]
    put = _up if path == "device" else (lambda a: None if a is None else np.array(a))
    radius, min_arm, min_cos = cfg
    return f.chain_joins(put(pts), put(table), xy=put(xy if with_xy else None), radius=radius, min_arm=min_arm, min_cos=min_cos)


@pytest.mark.parametrize("name", ["junctions", "random 0.20", "random 0.50"])
def test_joins_bit_for_bit(name):
    f = _filters()
    seen = 0
    for cfg in CONFIGS:
        for with_xy in (False, True):
            want = _want(name, with_xy, cfg)
            got = _call(f, name, with_xy, cfg, "device")
            assert got.dtype == M.JOIN_DTYPE and got.shape == (2 * len(_cases()[name][1]),)
            for field in M.JOIN_DTYPE.names:                                      # field by field first: a failure names it
                assert got[field].tobytes() == want[field].tobytes(), (cfg, with_xy, field, np.nonzero(got[field].view(np.int32) != want[field].view(np.int32))[0][:8])
            assert M.same_records(got, want), (cfg, with_xy)
            seen |= int(np.bitwise_or.reduce(want["flags"]))
    assert seen & M.MUTUAL and not seen & (M.NO_CHAIN | M.CROWDED)
    assert name == "junctions" or seen & M.SHORT                                # (the arms of the hand-made junctions have four points)
    cfg = (8, 3, -1.0)
    for with_xy in (False, True):                                                # the host path, and the same call twice
        want = _want(name, with_xy, cfg)
        a, b, c = _call(f, name, with_xy, cfg, "device"), _call(f, name, with_xy, cfg, "host"), _call(f, name, with_xy, cfg, "device")
        assert M.same_records(a, want) and M.same_records(b, want) and a.tobytes() == b.tobytes() == c.tobytes()
    want = _want(name, False, cfg)
    mutual = np.nonzero(want["flags"] & M.MUTUAL)[0]
    assert (want["partner"][want["partner"][mutual]] == mutual).all()           # an involution
    cos, sin = want["cos"].view(np.uint32), want["sin"].view(np.uint32)
    assert (cos[mutual] == cos[want["partner"][mutual]]).all() and ((sin[mutual] ^ sin[want["partner"][mutual]]) == 0x80000000).all()
    if name == "junctions":
        # the masks go through the library's own contour_chains
        mask = _junction_mask()
        d_pts, d_chains = f.contour_chains(_up(mask))
        assert np.array_equal(d_pts.cpu().numpy(), _cases()[name][0]) and np.array_equal(d_chains.cpu().numpy(), _cases()[name][1])
        got = f.chain_joins(d_pts, d_chains, radius=8)
        assert M.same_records(got, want)
        assert sorted(np.bincount(got["degree"][got["node"] == np.arange(len(got))]).tolist()) == [0, 0, 1, 2, 11]   # 11 free ends, a T, two crossings
        four = np.nonzero(got["degree"] == 4)[0]
        assert (got["flags"][four] == M.MUTUAL).all() and (got["cos"][four] == 1.0).all() and (got["sin"][four] == 0.0).all()
        three = np.nonzero(got["degree"] == 3)[0]
        assert sorted(got["flags"][three].tolist()) == [0, M.MUTUAL, M.MUTUAL] and got["partner"][three[2]] == three[0]
    else:
        live = want["degree"][want["node"] >= 0]
        assert not (live == 2).any() and live.max() <= 4


def test_batch_planes_never_join():
    """a batch table of three planes, the first and the last holding the same mask: the result is the per-plane results with the end
    numbers shifted, and no ring and no partner leaves its plane"""
    f = _filters()
    a = (np.random.default_rng(5).random((33, 65)) < 0.3).astype(F32)
    b = (np.random.default_rng(6).random((33, 65)) < 0.45).astype(F32)
    pts, chains, ranges = f.contour_chains_batch(_up(np.stack([a, b, a])))
    h_pts, h_chains, ranges = pts.cpu().numpy(), chains.cpu().numpy(), ranges.cpu().numpy()
    assert h_chains[:, 3].max() == 2 and (h_chains[:, 3] == 0).sum() == (h_chains[:, 3] == 2).sum() > 10
    xy = _jitter(h_pts)
    for sub in (None, xy):
        got = f.chain_joins(pts, chains, xy=_up(sub), radius=8)
        assert M.same_records(got, M.joins(h_pts, h_chains, sub, radius=8))
        planes = []
        for z in range(3):
            (c0, p0), (c1, p1) = ranges[z], ranges[z + 1]
            local = h_chains[c0:c1].copy()
            local[:, 0] -= p0
            local[:, 3] = 0
            one = f.chain_joins(_up(h_pts[p0:p1]), _up(local), xy=_up(None if sub is None else sub[p0:p1]), radius=8)
            part = got[2 * c0:2 * c1].copy()
            for field in ("node", "next", "partner"):
                part[field] = np.where(part[field] >= 0, part[field] - 2 * c0, -1)
            assert M.same_records(part, one), z
            planes.append(one)
            ends = np.nonzero(got["partner"][2 * c0:2 * c1] >= 0)[0] + 2 * c0
            assert (h_chains[got["partner"][ends] // 2, 3] == z).all() and (h_chains[got["next"][ends] // 2, 3] == z).all()
        if sub is None:
            assert planes[0].tobytes() == planes[2].tobytes() and planes[0].tobytes() != planes[1].tobytes()
    # the same pixels in ONE plane would meet: the plane word is what keeps them apart
    flat = h_chains.copy()
    flat[:, 3] = 0
    assert f.chain_joins(pts, _up(flat), radius=8)["degree"].max() > M.joins(h_pts, h_chains, radius=8)["degree"].max()


def test_crowded_nodes():
    """a hand-made device table of 8, then 9, two-point chains that all start at one pixel: degree 8 is resolved in full, degree 9 is
    CROWDED -- node and degree right, next = partner = -1, NaN"""
    f = _filters()
    spokes = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (2, 1)]
    for count in (8, 9):
        pts = np.int32([p for dx, dy in spokes[:count] for p in ((10, 10), (10 + dx, 10 + dy))])
        tab = np.int32([[2 * c, 2, 0, 0] for c in range(count)])
        for sub in (_jitter(pts), None):                                         # (the integer points last: they are looked at below)
            got = f.chain_joins(_up(pts), _up(tab), xy=_up(sub), radius=1, min_arm=1)
            assert M.same_records(got, M.joins(pts, tab, sub, radius=1, min_arm=1)), count
        heads = np.arange(0, 2 * count, 2)
        assert (got["node"][heads] == 0).all() and (got["degree"][heads] == count).all() and (got["degree"][heads + 1] == 1).all()
        if count == 8:
            assert got["next"][heads].tolist() == heads[1:].tolist() + [0] and (got["flags"][heads] & M.MUTUAL).all()
        else:
            assert (got["flags"][heads] == M.CROWDED).all() and (got["next"][heads] == -1).all() and (got["partner"][heads] == -1).all()
            assert (got["cos"].view(np.uint32)[heads] == M.QNAN_BITS).all() and (got["sin"].view(np.uint32)[heads] == M.QNAN_BITS).all()


def test_nan_in_xy_marks_its_arms():
    pts, chains, xy = _cases()["random 0.20"]
    radius = 8
    opened = np.nonzero(((chains[:, 2] & M.CLOSED) == 0) & (chains[:, 1] >= 2))[0]
    hit = [int(chains[opened[3], 0]), int(chains[opened[len(opened) // 2], 0] + chains[opened[len(opened) // 2], 1] - 1),
           int(chains[np.argmax(chains[:, 1]), 0] + chains[:, 1].max() // 2)]         # a head, a tail, the middle of the longest chain
    bad = np.array(xy)
    bad[hit, 0] = np.nan
    f = _filters()
    got = f.chain_joins(_up(pts), _up(chains), xy=_up(bad), radius=radius)
    assert M.same_records(got, M.joins(pts, chains, bad, radius=radius))
    clean = _want("random 0.20", True, (8, 3, -1.0))
    expect = []
    for c in opened:                                                            # the ends whose arm holds a NaN, from the contract
        s, ln = int(chains[c, 0]), int(chains[c, 1])
        n = min(radius, ln - 1)
        expect += [2 * c] if any(s <= p <= s + n for p in hit) else []
        expect += [2 * c + 1] if any(s + ln - 1 - n <= p <= s + ln - 1 for p in hit) else []
    marked = np.nonzero((got["flags"] & M.DEGENERATE) != 0)[0]
    assert marked.tolist() == sorted(expect) and len(marked) >= 2 and not (clean["flags"] & M.DEGENERATE).any()
    assert (got["partner"][marked] == -1).all() and (got["cos"].view(np.uint32)[marked] == M.QNAN_BITS).all()
    for field in ("node", "degree", "next", "n"):                               # who is where does not change
        assert np.array_equal(got[field], clean[field]), field
    apart = ~np.isin(got["node"], got["node"][marked])                          # and at every other node nothing changes at all
    assert apart.sum() > len(got) // 2 and got[apart].tobytes() == clean[apart].tobytes()


# ---- capture ----
def test_graph_capture():
    pts, chains, xy = (_up(a) for a in _cases()["random 0.20"])
    f = cv.SteerableFiltersG2(torch.zeros((33, 65), device=DEV))
    want = _want("random 0.20", True, (8, 3, -1.0))
    m = len(chains)
    tab = torch.empty((2 * m, 32), dtype=torch.uint8, device=DEV)
    big_chains = torch.cat([chains] * 8)                                        # eight times the chains: more scratch than the eager call left
    big_tab = torch.full((16 * m, 8), -9, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    p = lambda a: C.c_void_p(a.data_ptr() if torch.is_tensor(a) else a.ctypes.data)
    with torch.cuda.stream(side):
        f.chain_joins(pts, chains, xy=xy, out=tab)                              # the handle moves to the side stream outside the capture
        torch.cuda.synchronize()
        tab.fill_(7)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            assert f.chain_joins(pts, chains, xy=xy, out=tab) is tab
            hp, hc = np.int32([[0, 0], [1, 0]]), np.int32([[0, 2, 0, 0]])       # host arrays are refused while capturing
            ht = np.full((2, 8), -9, np.int32)
            cfg = L.JoinCfg(8, 3, -1.0, 0)
            rc_host = L.lib().cvs_chain_joins(f._h, p(hp), 2, p(hc), 1, None, C.byref(cfg), p(ht), L.MEM_HOST)
            rc_grow = L.lib().cvs_chain_joins(f._h, p(pts), len(pts), p(big_chains), 8 * m, p(xy), C.byref(cfg), p(big_tab), L.MEM_DEVICE)
            message = L.lib().cvs_last_error(f._h)
    assert rc_host == L.E_UNSUPPORTED and (ht == -9).all()
    assert rc_grow == L.E_UNSUPPORTED and b"call once eagerly first" in message
    torch.cuda.synchronize()
    assert bool((tab == 7).all()) and bool((big_tab == -9).all())               # a capture runs nothing
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert tab.cpu().numpy().view(M.JOIN_DTYPE).reshape(-1).tobytes() == want.tobytes()
        tab.fill_(7)
    assert bool((big_tab == -9).all())
    assert f.chain_joins(hp, hc, radius=1)["degree"].tolist() == [1, 1]         # the handle works on, on both paths
    assert M.same_records(f.chain_joins(pts, chains, xy=xy), want)
    h_pts, h_chains, h_xy = _cases()["random 0.20"]
    big = f.chain_joins(pts, big_chains, xy=xy)                                 # eagerly the larger table goes through: eight ends per pixel and more
    assert M.same_records(big, M.joins(h_pts, np.concatenate([h_chains] * 8), h_xy)) and np.bitwise_or.reduce(big["flags"]) & M.CROWDED


# ---- raw calls: guarded arrays, broken tables, errors ----
def _guarded(n, words):
    """(buffer, view): n records of `words` int32 words with GUARD records of sentinel in front and behind"""
    buf = torch.full((GUARD + n + GUARD, words), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _ptr(a):
    return None if a is None else C.c_void_p(a if isinstance(a, int) else (a.data_ptr() if torch.is_tensor(a) else a.ctypes.data))


def _raw(f, pts, n, chains, m, xy, cfg, table, mem):
    cfg = None if cfg is None else C.byref(L.JoinCfg(*cfg))
    return L.lib().cvs_chain_joins(f._h, _ptr(pts), n, _ptr(chains), m, _ptr(xy), cfg, _ptr(table), mem)


def test_broken_device_tables_give_no_chain_and_write_nothing_outside():
    pts, chains, xy = _cases()["random 0.20"]
    n, m = len(pts), len(chains)
    f = _filters()
    dp, dx = _up(pts), _up(xy)
    f._bind_stream(dp)
    negative, empty, long_, descending = (np.array(chains) for _ in range(4))
    negative[3, 0] = -1                                                         # a negative start
    negative[5, 0] = -2 ** 31
    empty[4, 1] = 0                                                             # no point, and a negative length
    empty[6, 1] = -3
    long_[-1, 1] += 1                                                           # the last chain leaves the array
    long_[2, 0], long_[7, 1] = 2 ** 31 - 1, 2 ** 31 - 1                         # sums past 2^31
    descending[:, 0] = descending[::-1, 0]                                      # starts that descend: entries that overlap, entries that leave
    for what, tab, count in (("negative starts", negative, 2), ("chains without a point", empty, 2), ("chains that leave the array", long_, 3),
                             ("descending starts", descending, 0)):
        tbuf, tview = _guarded(2 * m, 8)
        inputs = [torch.cat([torch.full((GUARD,) + a.shape[1:], 77, dtype=a.dtype, device=DEV), a, torch.full((GUARD,) + a.shape[1:], 77, dtype=a.dtype, device=DEV)])
                  for a in (dp, _up(tab), dx)]
        before = [a.clone() for a in inputs]
        gp, gc, gx = (a[GUARD:len(a) - GUARD] for a in inputs)
        assert _raw(f, gp, n, gc, m, gx, (8, 3, -1.0, 0), tview, L.MEM_DEVICE) == 0, what
        torch.cuda.synchronize()
        assert _guards_intact(tbuf, 2 * m), what
        assert all(torch.equal(a, b) for a, b in zip(inputs, before)), what     # no input is written
        got = tview.cpu().numpy().view(M.JOIN_DTYPE).reshape(-1)
        assert M.same_records(got, M.joins(pts, tab, xy)), what
        gone = np.nonzero(got["flags"] & M.NO_CHAIN)[0]
        assert len(gone) >= 2 * count and len(gone) % 2 == 0, what
        blank = np.zeros(1, M.JOIN_DTYPE)
        blank["node"] = blank["next"] = blank["partner"] = -1
        blank["flags"] = M.NONE | M.NO_CHAIN
        blank["sin"] = blank["cos"] = np.uint32(M.QNAN_BITS).view(F32)
        assert all(r.tobytes() == blank.tobytes() for r in got[gone]), what
        bad = ~((tab[:, 0].astype(np.int64) >= 0) & (tab[:, 1] >= 1) & (tab[:, 0].astype(np.int64) + tab[:, 1] <= n))
        assert gone.tolist() == sorted((2 * np.nonzero(bad)[0]).tolist() + (2 * np.nonzero(bad)[0] + 1).tolist()), what
        for field in ("node", "next", "partner"):                               # no record names an end of a broken entry
            assert not np.isin(got[field], gone).any(), (what, field)
        # the same table on the host is refused, and the output is untouched
        ht = np.full((2 * m, 8), -9, np.int32)
        keep = [np.array(pts), np.ascontiguousarray(tab), np.array(xy)]
        assert _raw(f, keep[0], n, keep[1], m, keep[2], (8, 3, -1.0, 0), ht, L.MEM_HOST) == L.E_BADARG, what
        assert (ht == -9).all(), what
        with pytest.raises(cv.CvsError) as ei:
            f.chain_joins(keep[0], keep[1], xy=keep[2])
        assert ei.value.status == L.E_BADARG


def test_errors_leave_the_output_untouched():
    pts, chains, xy = _cases()["random 0.20"]
    f = _filters()
    dp, dc, dx = (_up(a) for a in (pts, chains, xy))
    n, m, D, H, B = len(pts), len(chains), L.MEM_DEVICE, L.MEM_HOST, L.E_BADARG
    ok = (8, 3, -1.0, 0)
    tab = torch.full((2 * m + 1, 8), -9, dtype=torch.int32, device=DEV)
    f._bind_stream(dp)
    call = lambda p, n_, c, m_, x, cfg, t, mem: _raw(f, p, n_, c, m_, x, cfg, t, mem)
    # nothing to do: CVS_OK, nothing queued, nothing written
    assert call(None, 0, None, 0, None, ok, None, D) == 0 and call(None, 0, None, 0, None, ok, None, H) == 0
    assert call(dp, 0, dc, 0, dx, ok, tab, D) == 0
    # cfg
    assert call(dp, n, dc, m, dx, None, tab, D) == B
    for bad in ((0, 1, 0.5, 0), (65, 3, 0.5, 0), (-1, 1, 0.5, 0), (8, 0, 0.5, 0), (8, 9, 0.5, 0), (8, -1, 0.5, 0), (8, 3, float("nan"), 0),
                (8, 3, 1.5, 0), (8, 3, -1.5, 0), (8, 3, float("inf"), 0), (8, 3, 0.5, 1), (8, 3, 0.5, -1)):
        assert call(dp, n, dc, m, dx, bad, tab, D) == B, bad
    # counts, arrays, mem
    assert call(dp, -1, dc, m, dx, ok, tab, D) == B and call(dp, n, dc, -1, dx, ok, tab, D) == B
    assert call(None, n, dc, m, dx, ok, tab, D) == B and call(dp, n, None, m, dx, ok, tab, D) == B
    assert call(dp, n, dc, m, dx, ok, None, D) == B and call(dp, n, None, 0, dx, ok, tab, D) == B   # points without a chain
    assert call(dp, n, dc, m, dx, ok, tab, 5) == B and call(dp, n, dc, m, dx, ok, tab, -1) == B
    for k in range(4):                                                          # not aligned to 4 bytes
        args = [dp, dc, dx, tab]
        args[k] = args[k].data_ptr() + 2
        assert call(args[0], n, args[1], m, args[2], ok, args[3], D) == B, k
    for a in (dp, dc, dx):                                                      # the output over an input
        assert call(dp, n, dc, m, dx, ok, a, D) == B
    assert call(dp, n, dc.data_ptr() + 16 * (m - 1), 1, dx, ok, dc.data_ptr() + 16 * m - 32, D) == B   # its last record on the one entry
    assert call(dp, 2 ** 30 + 1, dc, m, None, ok, tab, D) == L.E_SIZE and call(dp, n, dc, 2 ** 26 + 1, dx, ok, tab, D) == L.E_SIZE
    # host tables that do not say what the contract says
    ht = np.full((2 * m, 8), -9, np.int32)
    host = lambda c, m_=m: call(np.array(pts), n, np.ascontiguousarray(c), m_, np.array(xy), ok, ht, H)
    for row, col, delta in ((-1, 1, 1), (-1, 1, -1), (0, 0, -1), (0, 0, 1), (1, 0, 1), (m // 2, 1, -int(chains[m // 2, 1]))):
        bad = np.array(chains)
        bad[row, col] += delta
        assert host(bad) == B, (row, col, delta)
    assert host(chains[:-1], m - 1) == B                                        # lengths that stop short of n_points
    assert call(None, 0, np.array(chains), m, None, ok, ht, H) == B             # chains without points
    torch.cuda.synchronize()
    assert bool((tab == -9).all()) and (ht == -9).all()
    # the same arrays unharmed: the calls go through, also into a table that is aligned to 4 bytes only
    want = M.joins(pts, chains, xy)
    assert host(chains) == 0 and ht.view(M.JOIN_DTYPE).reshape(-1).tobytes() == want.tobytes()
    flat = tab.reshape(-1)
    assert call(dp, n, dc, m, dx, ok, flat.data_ptr() + 4, D) == 0
    torch.cuda.synchronize()
    assert flat[1:1 + 16 * m].cpu().numpy().view(M.JOIN_DTYPE).tobytes() == want.tobytes() and int(flat[0]) == -9 and bool((flat[1 + 16 * m:] == -9).all())
    # device entries without a point to stand on: no points at all
    assert call(None, 0, dc, m, None, ok, tab, D) == 0
    torch.cuda.synchronize()
    assert (tab[:2 * m].cpu().numpy().view(M.JOIN_DTYPE).reshape(-1)["flags"] == (M.NONE | M.NO_CHAIN)).all()


# ---- end to end ----
def test_contour_joins_on_the_ridge_of_120_degrees():
    """the corner cvs_chain_turns cannot see: thinning cuts the ridge at its vertex, and the mutual join there puts it together again"""
    img, theta, (vx, vy), mask = TM.ridge_case(0.0, 120.0)
    f = cv.SteerableFiltersG2(_up(img))
    d_img, d_theta, d_mask = _up(img), _up(theta), _up(mask)
    pts, chains = CM.chains(mask)
    xy, _ = RM.refine(pts, img, theta)
    want = M.joins(pts, chains, xy, radius=8)
    joins, d_pts, d_chains, d_xy = f.contour_joins(d_mask, d_img, theta=d_theta, radius=8)
    assert np.array_equal(d_chains.cpu().numpy(), chains) and np.array_equal(d_pts.cpu().numpy(), pts) and d_xy.cpu().numpy().tobytes() == xy.tobytes()
    assert M.same_records(joins, want)
    at = np.nonzero(joins["flags"] & M.MUTUAL)[0]
    assert len(at) == 2 and joins["partner"][at].tolist() == at[::-1].tolist() and (joins["degree"][at] == 3).all()
    e = int(at[0])
    vertex = pts[chains[e // 2, 0] + (chains[e // 2, 1] - 1) * (e % 2)]
    assert np.hypot(vertex[0] - vx, vertex[1] - vy) <= 1.5 and -0.7 < joins["cos"][e] < -0.2   # the vertex pixel, a turn by about 120 degrees
    spur = int(np.argmin(chains[:, 1]))
    assert chains[spur, 1] == 3 and (joins["flags"][[2 * spur, 2 * spur + 1]] == M.SHORT).all()
    # the integer points, the configuration, the numpy path, out=
    assert M.same_records(f.chain_joins(d_pts, d_chains, radius=8), M.joins(pts, chains, radius=8))
    cfg = dict(radius=4, min_arm=1, min_cos=0.0)
    got = f.contour_joins(d_mask, d_img, theta=d_theta, **cfg)[0]
    assert M.same_records(got, M.joins(pts, chains, xy, **cfg)) and got["flags"][2 * spur] & M.MUTUAL or got["flags"][2 * spur + 1] & M.MUTUAL
    host = f.contour_joins(mask, img, theta=theta, radius=8)
    assert M.same_records(host[0], want) and isinstance(host[1], np.ndarray)
    tab = torch.empty((2 * len(chains), 32), dtype=torch.uint8, device=DEV)
    assert f.chain_joins(d_pts, d_chains, xy=d_xy, out=tab) is tab
    assert tab.cpu().numpy().view(M.JOIN_DTYPE).reshape(-1).tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        f.chain_joins(d_pts, d_chains, xy=d_xy, out=tab[:-1])


# ---- facade ----
def test_facade_member(tmp_path):
    exe = os.path.join(str(tmp_path), "test_joins")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_joins.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    img, _, _, mask = TM.ridge_case(0.0, 120.0)
    pts, table = CM.chains(mask)
    words = [len(table)]
    for s, n, fl, _ in table.tolist():
        words += [n, fl] + pts[s:s + n].reshape(-1).tolist()
    src_img, src, dst = (os.path.join(str(tmp_path), n) for n in ("image.f32", "chains.i32", "joins.f32"))
    np.ascontiguousarray(img, F32).tofile(src_img)
    np.array(words, np.int32).tofile(src)
    r = subprocess.run([exe, src_img, "48", "48", src, "8", "-1", dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dst, F32).reshape(-1, 2)                                  # partner, cos
    f = cv.SteerableFiltersG2(img)                                              # the facade's defaults: the same engine, its own theta
    xy, _ = f.chain_refine(pts, img)
    joins = f.chain_joins(pts, table, xy=xy, radius=8, min_arm=3, min_cos=-1.0)
    mutual = (joins["flags"] & M.MUTUAL) != 0
    assert "joins OK (%d chains, %d mutual joins)" % (len(table), mutual.sum() // 2) in r.stdout, r.stdout
    assert mutual.sum() >= 2 and got[:, 0].tolist() == np.where(mutual, joins["partner"], -1).tolist()
    assert got[mutual, 1].tobytes() == joins["cos"][mutual].tobytes() and np.isnan(got[~mutual, 1]).all()
