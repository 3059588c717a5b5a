"""GPU test (-m gpu): contour bridges -- cvs_chain_bridges, chain_bridges / contour_bridges and the facade's bridgeContours against the
model of bridges_model.py.

Every field of every record, every point, every chain entry and every sub-pixel position is held BIT FOR BIT: the arithmetic of an arm
and of a pair is sequential in one lane, in the order the contract names, a pair is evaluated from its smaller end by both ends, the
choice of the partner is an order on integers, and a bridge point is a function of (bridge, j) -- so there is no tolerance anywhere.
Two calls, the device and the host path, and a captured graph give the same bytes."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import bridges_cases as BC
import bridges_model as M
import chains_model as CM
import cvsteer_amd as cv
import joins_model as JM
import paths_model as PM
from cvsteer_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32 = np.float32
GUARD = 64
SENTINEL = 0x5A5A5A5A
DASHED = (8, 3, 4, 0.8)
_cache = {}


def _filters(shape=(33, 65)):
    if shape not in _cache:
        _cache[shape] = cv.SteerableFiltersG2(torch.zeros(shape, device=DEV))
    return _cache[shape]


def _up(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _arrays(name):
    if name == "two planes":
        return BC.two_planes()
    if name.startswith("moved "):
        return BC.shifted(name[6:], -17, -14)
    return BC.cases()[name]


@functools.lru_cache(maxsize=None)
def _want(name, with_xy, cfg, cap_points=None, cap_chains=None):
    pts, chains, xy = _arrays(name)
    radius, min_arm, max_gap, min_cos = cfg
    want = M.bridges(pts, chains, xy if with_xy else None, radius=radius, min_arm=min_arm, max_gap=max_gap, min_cos=min_cos,
                     cap_points=cap_points, cap_chains=cap_chains)
    for a in want[:4]:
        if a is not None:
            a.setflags(write=False)
    return want


def _call(f, name, with_xy, cfg, path, **kw):
    pts, table, xy = _arrays(name)
    put = _up if path == "device" else (lambda a: None if a is None else np.array(a))
    radius, min_arm, max_gap, min_cos = cfg
    return f.chain_bridges(put(pts), put(table), xy=put(xy if with_xy else None), radius=radius, min_arm=min_arm, max_gap=max_gap,
                           min_cos=min_cos, **kw)


def _host(a):
    return None if a is None else (a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a))


def _same(got, want, what):
    """(bridges, out_points, out_chains, out_xy) against the model's: field by field first, so that a failure names the field"""
    table, o_pts, o_chn, o_xy = (_host(a) for a in got)
    assert table.dtype == M.BRIDGE_DTYPE and table.shape == want[0].shape, what
    for field in M.BRIDGE_DTYPE.names:
        a, b = table[field].view(np.uint32), want[0][field].view(np.uint32)
        assert a.tobytes() == b.tobytes(), (what, field, np.nonzero(a != b)[0][:8], a[a != b][:4], b[a != b][:4])
    assert M.same_bytes("bridges", table, want[0])
    assert M.same_bytes("out_points", o_pts, want[1]) and M.same_bytes("out_chains", o_chn, want[2]), what
    assert (o_xy is None) == (want[3] is None), what
    assert o_xy is None or M.same_bytes("out_xy", o_xy.view(np.uint32), want[3].view(np.uint32)), what
    return True


# ---- the dashed figures ----
@pytest.mark.parametrize("kind", ["horizontal", "vertical", "diagonal"])
def test_dashed_lines(kind):
    f = _filters()
    dashes = BC.dashed_pixels(kind)[2]
    for with_xy in (False, True):
        want = _want(kind, with_xy, DASHED)
        assert want[4] == (dashes - 1, 2 * dashes - 1, len(want[1])) and len(want[1]) == len(_arrays(kind)[0]) + 5 * (dashes - 1)
        got = _call(f, kind, with_xy, DASHED, "device")
        assert _same(got, want, (kind, with_xy)) and all(torch.is_tensor(a) and a.is_cuda for a in got[1:3])
        assert _same(_call(f, kind, with_xy, DASHED, "host"), want, (kind, with_xy, "host"))
        none = _call(f, kind, with_xy, (8, 3, 2, 0.8), "device")
        assert _same(none, _want(kind, with_xy, (8, 3, 2, 0.8)), (kind, "max_gap 2")) and not (none[0]["flags"] & M.MUTUAL).any()
        assert len(none[1]) == len(_arrays(kind)[0])
    # through the library's own contour_chains, and the table alone
    d_pts, d_chains = f.contour_chains(_up(BC.dashed_mask(kind)))
    assert np.array_equal(_host(d_pts), _arrays(kind)[0]) and np.array_equal(_host(d_chains), _arrays(kind)[1])
    want = _want(kind, False, DASHED)
    assert _same(f.chain_bridges(d_pts, d_chains, radius=8, min_arm=3, max_gap=4, min_cos=0.8), want, kind)
    alone = f.chain_bridges(d_pts, d_chains, radius=8, min_arm=3, max_gap=4, min_cos=0.8, emit=False)
    assert alone[1:] == (None, None, None) and M.same_bytes("bridges", alone[0], want[0])


# ---- random masks: every configuration, both paths, twice ----
@pytest.mark.parametrize("name", ["random 0.05", "random 0.20"])
def test_random_masks_bit_for_bit(name):
    f = _filters()
    seen = 0
    for cfg in BC.CONFIGS:
        for with_xy in (False, True):
            want = _want(name, with_xy, cfg)
            assert _same(_call(f, name, with_xy, cfg, "device"), want, (cfg, with_xy))
            seen |= int(np.bitwise_or.reduce(want[0]["flags"]))
    assert seen & M.MUTUAL and seen & M.JUNCTION and seen & M.SHORT
    cfg = (8, 3, 5, 0.8)
    for with_xy in (False, True):                                                # the host path, and the same call twice
        want = _want(name, with_xy, cfg)
        a, b, c = (_call(f, name, with_xy, cfg, path) for path in ("device", "host", "device"))
        assert _same(a, want, "device") and _same(b, want, "host") and _same(c, want, "again")
        assert all(_host(x).tobytes() == _host(y).tobytes() == _host(z).tobytes() for x, y, z in zip(a, b, c) if x is not None)
        assert isinstance(b[1], np.ndarray)


def test_crowded_cells():
    """40 two-pixel chains in one 8 x 8 cell and 6 in its neighbour: all CROWDED at max_gap 8, while the dashes far away bridge; with
    cells of 2 x 2 nobody is crowded"""
    f = _filters()
    for cfg in ((1, 1, 8, 0.8), (1, 1, 8, -1.0), (1, 1, 2, -1.0), (1, 1, 32, -1.0)):
        for with_xy in (False, True):
            assert _same(_call(f, "crowd", with_xy, cfg, "device"), _want("crowd", with_xy, cfg), cfg)
    flags = _want("crowd", False, (1, 1, 8, 0.8))[0]["flags"]
    assert (flags[:92] == M.CROWDED).all() and flags[92:].tolist() == [0, M.MUTUAL, M.MUTUAL, 0] * 2
    assert not (_want("crowd", False, (1, 1, 2, -1.0))[0]["flags"] & M.CROWDED).any()


def test_batch_planes_never_bridge():
    f = _filters()
    pts, chains, xy = _arrays("two planes")
    for with_xy in (False, True):
        got = _call(f, "two planes", with_xy, DASHED, "device")
        assert _same(got, _want("two planes", with_xy, DASHED), with_xy)
        table = got[0]
        at = np.nonzero(table["partner"] >= 0)[0]
        assert len(at) == 24 and (chains[at // 2, 3] == chains[table["partner"][at] // 2, 3]).all()
        assert _host(got[2])[len(chains):, 3].tolist() == [0] * 6 + [1] * 6      # a bridge lies in the plane of its ends
    flat = np.array(chains)
    flat[:, 3] = 0                                                              # the same ends in ONE plane: ties go another way
    one = f.chain_bridges(_up(pts), _up(flat), radius=8, min_arm=3, max_gap=4, min_cos=0.8)
    assert _same(one, M.bridges(pts, flat, radius=8, min_arm=3, max_gap=4, min_cos=0.8), "flat")
    assert not np.array_equal(one[0]["partner"], _want("two planes", False, DASHED)[0]["partner"])


def test_negative_coordinates():
    f = _filters()
    for name in ("moved diagonal", "moved random 0.20"):
        pts = _arrays(name)[0]
        assert pts.min() < -8 and pts.max() > 8
        for cfg in ((8, 3, 5, 0.8), (8, 3, 32, -1.0)):
            for with_xy in (False, True):
                assert _same(_call(f, name, with_xy, cfg, "device"), _want(name, with_xy, cfg), (name, cfg, with_xy))
    assert (_want("moved diagonal", False, (8, 3, 5, 0.8))[0]["flags"] & M.MUTUAL).sum() == 4


# ---- raw calls: guarded arrays, arbitrary bytes, capacities, errors ----
def _guarded(n, words, dtype=torch.int32):
    """(buffer, view): n records of `words` 4-byte words with GUARD records of sentinel in front and behind"""
    buf = torch.full((GUARD + n + GUARD, words), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(dtype)


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _ptr(a):
    return None if a is None else C.c_void_p(a if isinstance(a, int) else (a.data_ptr() if torch.is_tensor(a) else a.ctypes.data))


def _raw(f, pts, n, chains, m, xy, cfg, table, o_pts, cap_p, o_chn, cap_c, o_xy, counts, mem):
    cfg = None if cfg is None else C.byref(L.BridgeCfg(*cfg))
    return L.lib().cvs_chain_bridges(f._h, _ptr(pts), n, _ptr(chains), m, _ptr(xy), cfg, _ptr(table), _ptr(o_pts), cap_p, _ptr(o_chn), cap_c,
                                     _ptr(o_xy), _ptr(counts), mem)


def _guarded_call(f, pts, chains, xy, cfg, cap_p, cap_c, what):
    """a DEVICE call on guarded copies of the arrays: returns (table, written out_points, out_chains, out_xy as the call left them --
    sentinel where nothing was written --, counts) and asserts that no input and no byte outside an output is touched"""
    n, m = len(pts), len(chains)
    ins = [torch.cat([torch.full((GUARD,) + a.shape[1:], 77, dtype=a.dtype, device=DEV), a, torch.full((GUARD,) + a.shape[1:], 77, dtype=a.dtype, device=DEV)])
           for a in (_up(pts), _up(chains), _up(xy if xy is not None else np.zeros((n, 2), F32)))]
    before = [a.clone() for a in ins]
    gp, gc, gx = (a[GUARD:len(a) - GUARD] for a in ins)
    (tb, tv), (pb, pv), (cb, cv_), (xb, xv), (nb, nv) = (_guarded(2 * m, 8), _guarded(cap_p, 2), _guarded(cap_c, 4), _guarded(cap_p, 2, torch.float32),
                                                           _guarded(1, 3))
    f._bind_stream(gp)
    assert _raw(f, gp, n, gc, m, gx if xy is not None else None, cfg, tv, pv, cap_p, cv_, cap_c, xv if xy is not None else None, nv, L.MEM_DEVICE) == 0, what
    torch.cuda.synchronize()
    assert all(_guards_intact(b, k) for b, k in ((tb, 2 * m), (pb, cap_p), (cb, cap_c), (xb, cap_p), (nb, 1))), what
    assert all(torch.equal(a, b) for a, b in zip(ins, before)), what             # no input is written
    assert xy is not None or bool((xv.view(torch.int32) == SENTINEL).all()), what
    return (tv.cpu().numpy().view(M.BRIDGE_DTYPE).reshape(-1), pv.cpu().numpy(), cv_.cpu().numpy(), xv.cpu().numpy() if xy is not None else None,
            tuple(nv.cpu().numpy().reshape(-1).tolist()))


def _check_written(got, want, what):
    """the prefix the model says is written equals it, everything behind it is still the sentinel, the counts are the full ones"""
    table, o_pts, o_chn, o_xy, counts = got
    q, k = len(want[1]), len(want[2])
    assert _same((table, o_pts[:q], o_chn[:k], None if o_xy is None else o_xy[:q]), want, what) and counts == want[4], (what, counts, want[4])
    assert (o_pts[q:].view(np.uint32) == SENTINEL).all() and (o_chn[k:].view(np.uint32) == SENTINEL).all(), what
    assert o_xy is None or (o_xy[q:].view(np.uint32) == SENTINEL).all(), what
    return True


def test_device_tables_of_arbitrary_bytes():
    f = _filters()
    rng = np.random.default_rng(11)
    pts, chains, xy = (np.array(a) for a in _arrays("random 0.20"))
    n, m = len(pts), len(chains)
    cfg = (8, 1, 5, -1.0)                                                       # (min_arm 1: the few pixels of the last case hold enough candidates to crowd)
    words = lambda shape: rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
    broken = chains.copy()                                                      # a third of the entries are random words
    hit = rng.choice(m, m // 3, replace=False)
    broken[hit] = words((len(hit), 4))
    broken[hit[::2], 0] = rng.integers(-4, n + 4, len(hit[::2]))                # some of them nearly chains: small starts and lengths
    broken[hit[::2], 1] = rng.integers(-2, 40, len(hit[::2]))
    wild_xy = xy.copy()
    wild_xy.view(np.uint32)[rng.choice(n, n // 8, replace=False)] = rng.integers(0, 2 ** 32, (n // 8, 2), dtype=np.uint64).astype(np.uint32)
    cases = (("broken entries", pts, broken, xy), ("random chain words", pts, words((m, 4)), None), ("random points", words((n, 2)), chains, None),
             ("xy of any bits", pts, broken, wild_xy), ("points in a few pixels", rng.integers(-3, 4, (n, 2)).astype(np.int32), chains, None))
    flags = 0
    for what, p, c, x in cases:
        want = M.bridges(p, c, x, radius=cfg[0], min_arm=cfg[1], max_gap=cfg[2], min_cos=cfg[3])
        got = _guarded_call(f, p, c, x, cfg, len(want[1]) + 3, len(want[2]) + 2, what)
        assert _check_written(got, want, what)
        flags |= int(np.bitwise_or.reduce(want[0]["flags"]))
    assert flags & M.NO_CHAIN and flags & M.DEGENERATE and flags & M.MUTUAL and flags & M.CROWDED
    # the broken table on the host is refused, and nothing is written
    ht, hc = np.full((2 * m, 8), -9, np.int32), np.full(3, -9, np.int32)
    assert _raw(f, pts, n, np.ascontiguousarray(broken), m, None, cfg, ht, None, 0, None, 0, None, hc, L.MEM_HOST) == L.E_BADARG
    assert (ht == -9).all() and (hc == -9).all()


def test_capacities_cut_after_the_first_bridge():
    f = _filters()
    pts, chains, xy = _arrays("horizontal")
    n, m = len(pts), len(chains)
    for cap_p, cap_c in ((n + 30, m + 1), (n + 9, m + 6), (n + 5, m + 1), (n + 4, m + 6), (n, m), (n + 30, m + 6), (n + 40, m + 9)):
        for with_xy in (False, True):
            want = _want("horizontal", with_xy, DASHED, cap_p, cap_c)
            fits = min(cap_c - m, (cap_p - n) // 5, 6)
            assert len(want[2]) == m + fits and len(want[1]) == n + 5 * fits and want[4] == (6, m + 6, n + 30)
            got = _guarded_call(f, pts, chains, xy if with_xy else None, DASHED, cap_p, cap_c, (cap_p, cap_c))
            assert _check_written(got, want, (cap_p, cap_c, with_xy))
            assert M.same_bytes("bridges", got[0], _want("horizontal", with_xy, DASHED)[0])   # the table does not see the capacities
            # the host path: the same prefix, the rest of the caller's arrays untouched
            ht, hp, hc, hx, hn = (np.full((2 * m, 8), -9, np.int32), np.full((cap_p, 2), SENTINEL, np.uint32).view(np.int32),
                                  np.full((cap_c, 4), SENTINEL, np.uint32).view(np.int32), np.full((cap_p, 2), SENTINEL, np.uint32).view(F32),
                                  np.full(3, -9, np.int32))
            assert _raw(f, np.array(pts), n, np.array(chains), m, np.array(xy) if with_xy else None, DASHED, ht, hp, cap_p, hc, cap_c,
                        hx if with_xy else None, hn, L.MEM_HOST) == 0
            assert _check_written((ht.view(M.BRIDGE_DTYPE).reshape(-1), hp, hc, hx if with_xy else None, tuple(hn.tolist())), want, "host")
    # chain_bridges with a capacity: what fitted
    got = _call(f, "horizontal", True, DASHED, "device", capacity=(n + 12, m + 6))
    assert _same(got, _want("horizontal", True, DASHED, n + 12, m + 6), "capacity") and len(got[2]) == m + 2


def test_graph_capture():
    pts, chains, xy = (_up(a) for a in _arrays("random 0.20"))
    f = cv.SteerableFiltersG2(torch.zeros((33, 65), device=DEV))
    cfg = (8, 3, 5, 0.8)
    want = _want("random 0.20", True, cfg)
    n, m = len(pts), len(chains)
    cap_p, cap_c = len(want[1]) + 7, len(want[2]) + 3
    new = lambda: (torch.empty((2 * m, 32), dtype=torch.uint8, device=DEV), torch.empty((cap_p, 2), dtype=torch.int32, device=DEV),
                   torch.empty((cap_c, 4), dtype=torch.int32, device=DEV), torch.empty((cap_p, 2), dtype=torch.float32, device=DEV),
                   torch.empty((3,), dtype=torch.int32, device=DEV))
    out = new()
    big_chains = torch.cat([chains] * 8)                                        # eight times the chains: more scratch than the eager call left
    big_tab = torch.full((16 * m, 8), -9, dtype=torch.int32, device=DEV)
    big_counts = torch.full((3,), -9, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    kw = dict(radius=cfg[0], min_arm=cfg[1], max_gap=cfg[2], min_cos=cfg[3])
    with torch.cuda.stream(side):
        f.chain_bridges(pts, chains, xy=xy, out=out, **kw)                      # the handle moves to the side stream outside the capture
        torch.cuda.synchronize()
        for t in out:
            t.view(torch.uint8).fill_(7)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            assert f.chain_bridges(pts, chains, xy=xy, out=out, **kw) is out
            hp, hc = np.int32([[0, 0], [1, 0]]), np.int32([[0, 2, 0, 0]])       # host arrays are refused while capturing
            ht, hn = np.full((2, 8), -9, np.int32), np.full(3, -9, np.int32)
            rc_host = _raw(f, hp, 2, hc, 1, None, cfg, ht, None, 0, None, 0, None, hn, L.MEM_HOST)
            rc_grow = _raw(f, pts, n, big_chains, 8 * m, xy, cfg, big_tab, None, 0, None, 0, None, big_counts, L.MEM_DEVICE)
            message = L.lib().cvs_last_error(f._h)
    assert rc_host == L.E_UNSUPPORTED and (ht == -9).all() and (hn == -9).all()
    assert rc_grow == L.E_UNSUPPORTED and b"call once eagerly first" in message
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == 7).all()) for t in out) and bool((big_tab == -9).all())   # a capture runs nothing
    q, k = len(want[1]), len(want[2])
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        table = out[0].cpu().numpy().view(M.BRIDGE_DTYPE).reshape(-1)
        assert _same((table, out[1][:q], out[2][:k], out[3][:q]), want, "replay") and tuple(out[4].tolist()) == want[4]
        assert bool((out[1][q:].view(torch.uint8) == 7).all()) and bool((out[2][k:].view(torch.uint8) == 7).all())
        for t in out:
            t.view(torch.uint8).fill_(7)
    assert bool((big_tab == -9).all()) and bool((big_counts == -9).all())
    got = f.chain_bridges(hp, hc, radius=1, min_arm=1, max_gap=2)               # the handle works on, on both paths
    assert got[0]["flags"].tolist() == [0, 0] and np.array_equal(got[1], hp) and np.array_equal(got[2], hc)
    assert _same(f.chain_bridges(pts, chains, xy=xy, **kw), want, "eager")
    h_pts, h_chains, h_xy = _arrays("random 0.20")
    big = f.chain_bridges(pts, big_chains, xy=xy, emit=False, **kw)[0]          # eagerly the larger table goes through
    assert M.same_bytes("bridges", big, M.bridges(h_pts, np.concatenate([h_chains] * 8), h_xy, **kw)[0])
    with pytest.raises(ValueError):
        f.chain_bridges(pts, chains, xy=xy, out=out[:3] + out[4:], **kw)


def test_errors_leave_the_outputs_untouched():
    pts, chains, xy = _arrays("horizontal")
    f = _filters()
    dp, dc, dx = (_up(a) for a in (pts, chains, xy))
    n, m, D, H, B = len(pts), len(chains), L.MEM_DEVICE, L.MEM_HOST, L.E_BADARG
    ok = DASHED
    cp, cc = n + 30, m + 6
    tab = torch.full((2 * m + 1, 8), -9, dtype=torch.int32, device=DEV)
    op, oc = torch.full((cp + 1, 2), -9, dtype=torch.int32, device=DEV), torch.full((cc + 1, 4), -9, dtype=torch.int32, device=DEV)
    ox, cnt = torch.full((cp + 1, 2), -9.0, dtype=torch.float32, device=DEV), torch.full((4,), -9, dtype=torch.int32, device=DEV)
    f._bind_stream(dp)
    good = dict(p=dp, n=n, c=dc, m=m, x=dx, cfg=ok, t=tab, op=op, cp=cp, oc=oc, cc=cc, ox=ox, k=cnt, mem=D)

    def call(**kw):
        a = dict(good, **kw)
        return _raw(f, a["p"], a["n"], a["c"], a["m"], a["x"], a["cfg"], a["t"], a["op"], a["cp"], a["oc"], a["cc"], a["ox"], a["k"], a["mem"])

    # nothing to do: counts = (0, 0, 0)
    zero = torch.full((3,), 5, dtype=torch.int32, device=DEV)
    assert call(p=None, n=0, c=None, m=0, x=None, t=None, op=None, cp=0, oc=None, cc=0, ox=None, k=zero) == 0
    hz = np.full(3, 5, np.int32)
    assert call(p=None, n=0, c=None, m=0, x=None, t=None, op=None, cp=0, oc=None, cc=0, ox=None, k=hz, mem=H) == 0
    torch.cuda.synchronize()
    assert zero.tolist() == [0, 0, 0] and hz.tolist() == [0, 0, 0]
    # cfg
    assert call(cfg=None) == B
    for bad in ((0, 1, 4, 0.5), (65, 3, 4, 0.5), (-1, 1, 4, 0.5), (8, 0, 4, 0.5), (8, 9, 4, 0.5), (8, -1, 4, 0.5), (8, 3, 1, 0.5), (8, 3, 0, 0.5),
                (8, 3, 33, 0.5), (8, 3, -4, 0.5), (8, 3, 4, float("nan")), (8, 3, 4, 1.5), (8, 3, 4, -1.5), (8, 3, 4, float("inf"))):
        assert call(cfg=bad) == B, bad
    # counts, arrays, capacities, mem
    assert call(n=-1) == B and call(m=-1) == B and call(k=None) == B
    assert call(p=None) == B and call(c=None) == B and call(t=None) == B and call(c=None, m=0) == B   # (the last: points without a chain)
    assert call(op=None) == B and call(oc=None) == B                            # both or neither
    assert call(op=None, oc=None, ox=None, cp=cp, cc=0) == B and call(op=None, oc=None, ox=None, cp=0, cc=cc) == B   # a capacity without its array
    assert call(cp=n - 1) == B and call(cc=m - 1) == B and call(cp=-1) == B
    assert call(ox=None) == B and call(x=None) == B and call(op=None, oc=None, cp=0, cc=0) == B   # out_xy: iff xy and out_points
    assert call(mem=5) == B and call(mem=-1) == B
    for key in ("p", "c", "x", "t", "op", "oc", "ox", "k"):                     # not aligned to 4 bytes
        assert call(**{key: good[key].data_ptr() + 2}) == B, key
    for key in ("t", "op", "oc", "ox", "k"):                                     # an output over an input, or over another output
        assert call(**{key: dp}) == B, key
    assert call(k=tab) == B and call(ox=op) == B and call(oc=tab) == B
    assert call(n=2 ** 30 + 1, x=None, ox=None, cp=2 ** 31 - 1) == L.E_SIZE and call(m=2 ** 26 + 1, cc=2 ** 26 + 1) == L.E_SIZE
    # host tables that do not say what the contract says
    ht, hp, hc, hn = np.full((2 * m, 8), -9, np.int32), np.full((cp, 2), -9, np.int32), np.full((cc, 4), -9, np.int32), np.full(3, -9, np.int32)
    host = lambda c, m_=m: call(p=np.array(pts), c=np.ascontiguousarray(c), m=m_, x=None, t=ht, op=hp, oc=hc, ox=None, k=hn, mem=H)
    for row, col, delta in ((-1, 1, 1), (-1, 1, -1), (0, 0, -1), (0, 0, 1), (1, 0, 1), (m // 2, 1, -int(chains[m // 2, 1]))):
        bad = np.array(chains)
        bad[row, col] += delta
        assert host(bad) == B, (row, col, delta)
    assert host(chains[:-1], m - 1) == B                                        # lengths that stop short of n_points
    torch.cuda.synchronize()
    assert all(bool((t == -9).all()) for t in (tab, op, oc, ox, cnt)) and all((a == -9).all() for a in (ht, hp, hc, hn))
    # the same arrays unharmed: the calls go through, also into a table that is aligned to 4 bytes only
    want = _want("horizontal", False, DASHED)
    assert host(chains) == 0 and _same((ht.view(M.BRIDGE_DTYPE).reshape(-1), hp, hc, None), want, "host") and tuple(hn.tolist()) == want[4]
    flat = tab.reshape(-1)
    assert call(t=flat.data_ptr() + 4) == 0
    torch.cuda.synchronize()
    want = _want("horizontal", True, DASHED)
    assert flat[1:1 + 16 * m].cpu().numpy().view(M.BRIDGE_DTYPE).tobytes() == want[0].tobytes() and int(flat[0]) == -9 and bool((flat[1 + 16 * m:] == -9).all())
    assert _same((want[0], op[:cp], oc[:cc], ox[:cp]), want, "device") and cnt.tolist() == list(want[4]) + [-9]
    assert bool((op[cp:] == -9).all()) and bool((oc[cc:] == -9).all()) and bool((ox[cp:] == -9).all())


# ---- end to end ----
@pytest.mark.parametrize("kind", ["horizontal", "vertical", "diagonal"])
def test_contour_bridges_gives_one_path_per_dashed_line(kind):
    f = _filters()
    mask = BC.dashed_mask(kind)
    whole = BC.dashed_pixels(kind)[1]
    pts, chains = CM.chains(mask)
    first = PM.paths(pts, chains, JM.joins(pts, chains, radius=8, min_arm=3))
    _, b_pts, b_chn, _, _ = M.bridges(first["path_points"], first["paths"], radius=8, min_arm=3, max_gap=4, min_cos=0.8)
    want = PM.paths(b_pts, b_chn, JM.joins(b_pts, b_chn, radius=8, min_arm=2))
    assert want["counts"] == (1, len(whole)) and list(map(tuple, want["path_points"].tolist())) == whole
    for put in (_up, np.array):
        path_points, paths, members, info = f.contour_bridges(put(mask), radius=8, min_arm=3, max_gap=4, min_cos=0.8)
        assert PM.same_bytes("path_points", _host(path_points), want["path_points"]) and PM.same_bytes("paths", _host(paths), want["paths"])
        assert PM.same_bytes("members", members, want["members"]) and PM.same_bytes("info", info, want["info"])
    apart = f.contour_bridges(_up(mask), radius=8, min_arm=3, max_gap=2, min_cos=0.8)
    assert len(apart[1]) == BC.dashed_pixels(kind)[2]                            # no bridge, no stitching: the dashes


# ---- facade ----
def test_facade_member(tmp_path):
    exe = os.path.join(str(tmp_path), "test_bridges")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_bridges.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bridges OK (7 dashes, 6 bridges, 1 path of 60 points)" in r.stdout, r.stdout + r.stderr
