"""GPU test (-m gpu): contour edgels -- cvs_chain_refine and cvs_chain_measures, chain_refine / chain_measures / contour_edgels and the
facade's refineContours against the models of refine_model.py.

Two tiers for the positions.  With theta == 0 the kernel's and the oracle's (cos, sin) are both exactly (1, 0), so xy and strength are held
to the float32 model BIT FOR BIT.  With a random theta the kernel's polynomial sincos may differ from the oracle's in the last bits, so that
tier uses the tolerance the issue sets: at the kept points that contour_model.decided accepts and whose a + b exceeds 1e-3 (|m| + |vb| +
|vf|), |delta| <= K 2^-23 (|m| + |vb| + |vf|) / (a + b); K comes from the model alone (see _tier_k).  The measures compare exactly in their
integer fields, peak, weakest and peak_index, and within (L + 2) 2^-52 sum|terms| -- the bound of L correctly rounded additions -- in sum
and length."""
import ctypes as C
import functools
import os
import subprocess
import time

import numpy as np
import pytest
import torch

import chains_model as CM
import contour_model as NM
import cvsteer_amd as cv
import refine_model as M
from cvsteer_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32 = np.float32
EPS = 2.0 ** -23
TIER_SHAPES = ((33, 65), (64, 200), (7, 130))
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _np(t):
    return t.cpu().numpy() if torch.is_tensor(t) else t


def _filters(shape):
    """a G2 object whose image size is `shape` (the setup image is zeros: the tests pass theta explicitly unless they say otherwise)"""
    if shape not in _cache:
        _cache[shape] = cv.SteerableFiltersG2(torch.zeros(shape, device=DEV))
    return _cache[shape]


@functools.lru_cache(maxsize=None)
def _case(shape, seed, zero_theta=False):
    rng = np.random.default_rng(seed)
    m = rng.random(shape, dtype=F32)
    theta = np.zeros(shape, F32) if zero_theta else (np.pi - 2 * np.pi * rng.random(shape)).astype(F32)   # (-pi, pi]
    for a in (m, theta):
        a.setflags(write=False)
    return m, theta


def _nudge(v, k):
    out = np.array(v, F32)
    for _ in range(abs(k)):
        out = np.nextafter(out, F32(np.inf if k > 0 else -np.inf))
    return out


def _accepted(P):
    """the kept points of the tolerance tier, and those among them the bound applies to"""
    with np.errstate(all="ignore"):
        scale = np.abs(P["m"]) + np.abs(P["vb"]) + np.abs(P["vf"])
        curve = P["a"] + P["b"]
        ok = NM.decided(P["m"], P["vb"], P["vf"]) & (curve > F32(1e-3) * scale) & P["keep"]
    return P["keep"], ok, scale.astype(np.float64), curve.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _tier_k():
    """K of the tolerance tier, from the model alone: the float32 model with c and s each nudged by -2, 0, +2 ulp against the model on
    the oracle's own (c, s), the largest quotient |delta| (a + b) / (2^-23 (|m| + |vb| + |vf|)) over the accepted points of the three tier
    inputs (for the strength, which carries no division: |delta| / (2^-23 (|m| + |vb| + |vf|))), times 4 for margin.  Measured on a CPU:
    quotients 110.4 (positions) and 1.51 (strength), so K = 441 and 6.04; the absolute deviations of the positions under these nudges are
    3.8e-6, 1.5e-5 and 7.6e-6 px on the three inputs -- one ulp of a float32 position at x ~ 60, 190 and 120, which is why the quotient of
    the positions is large where a + b is -- and the model excludes 0 of 851, 4744 and 386 kept points."""
    q_xy = q_st = 0.0
    for shape in TIER_SHAPES:
        m, theta = _case(shape, 11)
        c, s = M.directions(theta)
        P = M.refine_map(m, c, s)
        kept, ok, scale, curve = _accepted(P)
        for dc in (-2, 0, 2):
            for ds in (-2, 0, 2):
                Q = M.refine_map(m, _nudge(c, dc), _nudge(s, ds))
                both = ok & _accepted(Q)[1]
                for name in ("xs", "ys"):
                    d = np.abs(Q[name].astype(np.float64) - P[name])[both]
                    q_xy = max(q_xy, float((d * curve[both] / (EPS * scale[both])).max()))
                d = np.abs(Q["strength"].astype(np.float64) - P["strength"])[both]
                q_st = max(q_st, float((d / (EPS * scale[both])).max()))
    return 4.0 * q_xy, 4.0 * q_st


def _refine(f, points, m, theta, path, strength=True):
    """chain_refine on one path -> numpy (xy, strength)"""
    if path == "device":
        up = lambda a: None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
        xy, st = f.chain_refine(up(np.asarray(points, np.int32)), up(m), up(theta))
        assert xy.is_cuda and xy.dtype == torch.float32 and st.is_cuda
    else:
        xy, st = f.chain_refine(np.asarray(points, np.int32), _np(m), None if theta is None else _np(theta))
        assert isinstance(xy, np.ndarray) and xy.dtype == F32 and isinstance(st, np.ndarray)
    return _np(xy), _np(st)


def _border_points(rows, cols):
    edge = [(x, y) for y in (0, rows - 1) for x in range(cols)] + [(x, y) for x in (0, cols - 1) for y in range(rows)]
    return edge + [(0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1)]


# ---- tier 1: theta == 0, bit for bit ----
@pytest.mark.parametrize("path", ["device", "host"])
@pytest.mark.parametrize("layout", ["dense", "pitched"])
def test_theta_zero_is_the_model_bit_for_bit(layout, path):
    shape = (33, 65)
    m, theta = _case(shape, 3, True)
    c, s = M.directions(theta)
    assert (c == 1).all() and (s == 0).all()
    P = M.refine_map(m, c, s)
    rng = np.random.default_rng(4)
    ky, kx = np.nonzero(P["keep"])
    ny, nx = np.nonzero(~P["keep"])
    pick = rng.choice(len(ny), 300, replace=False)
    points = np.array(list(zip(kx, ky)) + list(zip(nx[pick], ny[pick])) + _border_points(*shape), np.int32)
    assert len(kx) > 300
    want_xy, want_st = M.gather(P, points)
    f = _filters(shape)
    if layout == "pitched":                                                     # column windows of wider buffers, NaN around them
        if path == "device":
            wide = torch.full((2, shape[0], shape[1] + 11), float("nan"), device=DEV)
            wide[0, :, 3:3 + shape[1]] = torch.from_numpy(np.array(m)).to(DEV)
            wide[1, :, 3:3 + shape[1]] = 0.0
        else:
            wide = np.full((2, shape[0], shape[1] + 11), np.nan, F32)
            wide[0, :, 3:3 + shape[1]], wide[1, :, 3:3 + shape[1]] = m, 0.0
        mm, tt = wide[0, :, 3:3 + shape[1]], wide[1, :, 3:3 + shape[1]]
    else:
        mm, tt = np.array(m), np.array(theta)
    xy, st = _refine(f, points, mm, tt, path)
    assert np.array_equal(_bits(xy), _bits(want_xy)), int((_bits(xy) != _bits(want_xy)).any(axis=1).sum())
    assert np.array_equal(_bits(st), _bits(want_st)), int((_bits(st) != _bits(want_st)).sum())
    moved = (xy != points).any(axis=1)
    assert moved[:len(kx)].sum() > 0.9 * len(kx) and not moved[len(kx):len(kx) + 300].any()   # kept points move, the others stay


# ---- tier 2: random theta, the issue's tolerance ----
def _check_tolerance(P, points, xy, st, what, max_excluded=0.02):
    kxy, kst = _tier_k()
    kept, ok, scale, curve = _accepted(P)
    x, y = points[:, 0], points[:, 1]
    assert kept[y, x].all()
    ok, scale, curve = ok[y, x], scale[y, x], curve[y, x]
    want_xy, want_st = M.gather(P, points)
    d_xy = np.abs(xy.astype(np.float64) - want_xy).max(axis=1)
    d_st = np.abs(st.astype(np.float64) - want_st)
    excluded = int((~ok).sum())
    q_xy = float((d_xy[ok] * curve[ok] / (EPS * scale[ok])).max())
    q_st = float((d_st[ok] / (EPS * scale[ok])).max())
    print("%s: %d kept points, %d excluded; positions: max |delta| %.3g px, quotient %.3g (K %.3g); strength: quotient %.3g (K %.3g)"
          % (what, len(points), excluded, float(d_xy[ok].max()), q_xy, kxy, q_st, kst))
    assert excluded <= max_excluded * len(points)
    assert (d_xy[ok] <= kxy * EPS * scale[ok] / curve[ok]).all() and (d_st[ok] <= kst * EPS * scale[ok]).all()
    assert np.isfinite(xy).all() and np.isfinite(st).all()
    assert (np.abs(xy[:, 0] - x) <= 0.5).all() and (np.abs(xy[:, 1] - y) <= 0.5).all()       # every point, the excluded ones included


@pytest.mark.parametrize("shape", TIER_SHAPES)
def test_random_theta_within_the_tolerance(shape):
    m, theta = _case(shape, 11)
    P = M.refine_map(m, *M.directions(theta))
    ky, kx = np.nonzero(P["keep"])
    points = np.stack([kx, ky], axis=1).astype(np.int32)
    assert len(points) > 100
    xy, st = _refine(_filters(shape), points, np.array(m), np.array(theta), "device")
    _check_tolerance(P, points, xy, st, "random theta %d x %d" % shape)
    hxy, hst = _refine(_filters(shape), points, np.array(m), np.array(theta), "host")
    assert np.array_equal(_bits(hxy), _bits(xy)) and np.array_equal(_bits(hst), _bits(st))     # one kernel behind both paths


# ---- edge shapes ----
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1)])
def test_tiny_images_and_point_counts(shape):
    rows, cols = shape
    m, theta = _case(shape, 21, True)
    P = M.refine_map(m, *M.directions(theta))
    f = _filters(shape)
    rng = np.random.default_rng(22)
    dm, dt = torch.from_numpy(np.array(m)).to(DEV), torch.from_numpy(np.array(theta)).to(DEV)
    for n in (0, 1, 63, 64, 65, 257):
        points = np.stack([rng.integers(0, cols, n), rng.integers(0, rows, n)], axis=1).astype(np.int32)
        want_xy, want_st = M.gather(P, points)
        for path in ("device", "host"):
            xy, st = _refine(f, points, dm if path == "device" else np.array(m), dt if path == "device" else np.array(theta), path)
            assert xy.shape == (n, 2) and st.shape == (n,)
            assert np.array_equal(_bits(xy), _bits(want_xy)) and np.array_equal(_bits(st), _bits(want_st)), (n, path)
    # device points one step outside the image: NaN triples, their neighbours in the list untouched
    points = np.stack([rng.integers(0, cols, 65), rng.integers(0, rows, 65)], axis=1).astype(np.int32)
    for k, p in ((3, (-1, 0)), (17, (cols, 0)), (40, (0, rows)), (63, (0, -1)), (64, (cols, rows))):
        points[k] = p
    want_xy, want_st = M.gather(P, points)
    assert np.isnan(want_st).sum() == 5
    xy, st = _refine(f, points, dm, dt, "device")
    assert np.array_equal(_bits(xy), _bits(want_xy)) and np.array_equal(_bits(st), _bits(want_st))
    assert np.isnan(xy[[3, 17, 40, 63, 64]]).all() and np.isfinite(xy[[2, 4, 16, 18, 39, 41, 62]]).all()


# ---- state and streams ----
def _kept_points(f, maps, n=400):
    thin = f.nonmax(maps)
    yx = torch.nonzero(thin > 0)[:n]
    return torch.stack([yx[:, 1], yx[:, 0]], dim=1).to(torch.int32).contiguous()


def test_own_theta_streams_and_a_frame_of_a_batch():
    from helpers import rand_image
    img = torch.from_numpy(rand_image(64, 200, seed=5)).to(DEV)
    f = cv.SteerableFiltersG2(img)
    edges = f.pipeline(img)[5]
    pts = _kept_points(f, edges)
    assert len(pts) > 50
    own = f.chain_refine(pts, edges)
    explicit = f.chain_refine(pts, edges, f.getDominantOrientationAngle())
    assert torch.equal(own[0], explicit[0]) and torch.equal(own[1], explicit[1])
    assert bool(torch.isfinite(own[0]).all()) and bool(((own[0] - pts).abs() <= 0.5).all()) and bool((own[0] != pts).any())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again = f.chain_refine(pts, edges)
    side.synchronize()
    assert torch.equal(again[0], own[0]) and torch.equal(again[1], own[1])
    # the selected frame of a batch
    frames = torch.stack([torch.from_numpy(rand_image(64, 200, seed=s)) for s in range(3)]).to(DEV)
    fb = cv.SteerableFiltersG2(frames[0])
    out = fb.pipeline_batch(frames)
    fb.select_frame(2)
    e2 = out[2, 5]
    p2 = _kept_points(fb, e2)
    own2 = fb.chain_refine(p2, e2)
    exp2 = fb.chain_refine(p2, e2, fb.getDominantOrientationAngle())
    assert torch.equal(own2[0], exp2[0]) and torch.equal(own2[1], exp2[1])
    fb.select_frame(0)
    other = fb.chain_refine(p2, e2)
    assert not torch.equal(other[0], own2[0])


def test_graph_capture_of_both_calls():
    from helpers import rand_image
    img = torch.from_numpy(rand_image(64, 200, seed=6)).to(DEV)
    f = cv.SteerableFiltersG2(img)
    edges = f.pipeline(img)[5]
    mask = f.hysteresis(f.nonmax(edges), 0.0, 0.0)
    pts, chains = f.contour_chains(mask)
    assert len(chains) > 10
    want_xy, want_st = f.chain_refine(pts, edges)
    want_tab = f.chain_measures(pts, chains, strength=want_st, xy=want_xy)
    xy, st = torch.empty_like(want_xy), torch.empty_like(want_st)
    tab = torch.empty((len(chains), 40), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f.chain_refine(pts, edges, out=(xy, st))               # the handle moves to the side stream outside the capture
        torch.cuda.synchronize()
        xy.fill_(7.0), st.fill_(7.0), tab.fill_(7)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            f.chain_refine(pts, edges, out=(xy, st))
            f.chain_measures(pts, chains, strength=st, xy=xy, out=tab)
            # host arrays are refused while capturing
            hp = np.zeros((1, 2), np.int32)
            hxy = np.full((1, 2), -9, F32)
            pm = cv.api._plane(edges)
            rc = L.lib().cvs_chain_refine(f._h, C.byref(pm), None, C.c_void_p(hp.ctypes.data), 1, C.c_void_p(hxy.ctypes.data), None, L.MEM_HOST)
            ht = np.full((1, 10), -9, np.int32)
            hc = np.int32([[0, 1, 0, 0]])
            rc2 = L.lib().cvs_chain_measures(f._h, C.c_void_p(hp.ctypes.data), 1, C.c_void_p(hc.ctypes.data), 1, None, None,
                                             C.c_void_p(ht.ctypes.data), L.MEM_HOST)
    assert rc == L.E_UNSUPPORTED and rc2 == L.E_UNSUPPORTED and (hxy == -9).all() and (ht == -9).all()
    torch.cuda.synchronize()
    assert bool((xy == 7.0).all()) and bool((tab == 7).all())                 # a capture runs nothing
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(xy, want_xy) and torch.equal(st, want_st)
    assert tab.cpu().numpy().view(M.MEASURE_DTYPE).reshape(-1).tobytes() == want_tab.tobytes()


# ---- measures ----
def _pack(lists, flags):
    pts = np.concatenate(lists).astype(np.int32).reshape(-1, 2)
    table, start = [], 0
    for p, fl in zip(lists, flags):
        table.append((start, len(p), fl, 0))
        start += len(p)
    return pts, np.array(table, np.int32).reshape(-1, 4)


def _walk(n, seed):
    """n points of a king's walk: every step goes to an 8-neighbour"""
    rng = np.random.default_rng(seed)
    steps = np.array([(1, 0), (1, 1), (0, 1), (1, -1)])[rng.integers(0, 4, max(n - 1, 0))]
    return np.concatenate([[[3, 500]], [3, 500] + np.cumsum(steps, axis=0)]).astype(np.int32) if n > 1 else np.int32([[3, 500]])


@functools.lru_cache(maxsize=None)
def _measure_cases():
    cases = {}
    for density in (0.15, 0.5):
        mask = (np.random.default_rng(int(100 * density)).random((33, 65)) < density).astype(F32)
        cases["random %.2f" % density] = CM.chains(mask)
    ring = [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (3, 2), (3, 3), (2, 3), (1, 3), (0, 3), (0, 2), (0, 1)]
    lens = (1, 2, 64, 65, 256, 257, 1000)
    lists = [_walk(n, n) for n in lens] + [np.int32(ring), np.int32([[7, 7]]), _walk(300, 9), np.int32([[0, 0], [5, 9], [5, 9]])]
    flags = [0] * len(lens) + [CM.CLOSED, 0, CM.CLOSED, CM.CLOSED]           # a ring, an isolated point, a long cycle, steps of kind `other`
    cases["hand made"] = _pack(lists, flags)
    out = {}
    for name, (pts, chains) in cases.items():
        rng = np.random.default_rng(len(pts))
        strength = rng.standard_normal(len(pts)).astype(F32)
        strength[rng.random(len(pts)) < 0.03] = np.nan
        strength[rng.random(len(pts)) < 0.03] = strength[0]                    # equal peaks: the first one counts
        xy = (pts + rng.uniform(-0.5, 0.5, pts.shape)).astype(F32)
        for a in (pts, chains, strength, xy):
            a.setflags(write=False)
        out[name] = (pts, chains, strength, xy)
    return out


@functools.lru_cache(maxsize=None)
def _measure_want(name, with_strength, with_xy):
    pts, chains, strength, xy = _measure_cases()[name]
    return M.measures(pts, chains, strength if with_strength else None, xy if with_xy else None, return_abs=True)


def _check_measures(got, want, abs_sum, abs_len, chains):
    for field in ("axial", "diagonal", "other", "peak_index"):
        assert np.array_equal(got[field], want[field]), field
    assert np.array_equal(_bits(got["peak"]), _bits(want["peak"])) and np.array_equal(_bits(got["weakest"]), _bits(want["weakest"]))
    n = chains[:, 1].astype(np.float64)
    nan = np.isnan(want["sum"])
    assert np.array_equal(np.isnan(got["sum"]), nan)
    assert (np.abs(got["sum"] - want["sum"])[~nan] <= ((n + 2) * 2.0 ** -52 * abs_sum)[~nan]).all()
    assert (np.abs(got["length"] - want["length"]) <= (n + 2) * 2.0 ** -52 * abs_len).all()


@pytest.mark.parametrize("path", ["device", "host"])
@pytest.mark.parametrize("name", ["random 0.15", "random 0.50", "hand made"])
def test_measures(name, path):
    pts, chains, strength, xy = _measure_cases()[name]
    f = _filters((33, 65))
    up = (lambda a: torch.from_numpy(np.array(a)).to(DEV)) if path == "device" else np.array
    for with_strength, with_xy in ((True, True), (False, False), (True, False), (False, True)):
        want, abs_sum, abs_len = _measure_want(name, with_strength, with_xy)
        args = (up(pts), up(chains), up(strength) if with_strength else None, up(xy) if with_xy else None)
        got = f.chain_measures(*args)
        assert isinstance(got, np.ndarray) and got.dtype == M.MEASURE_DTYPE and got.shape == (len(chains),)
        _check_measures(got, want, abs_sum, abs_len, chains)
        assert f.chain_measures(*args).tobytes() == got.tobytes()               # two calls: identical bytes
        if not with_strength:
            assert (got["peak_index"] == -1).all() and np.isneginf(got["peak"]).all() and np.isposinf(got["weakest"]).all() and not got["sum"].any()
    if name == "hand made":
        assert int(chains[:, 1].max()) == 1000 and got["other"].sum() > 0


def test_a_bad_entry_of_a_device_table_is_an_empty_record():
    pts, chains, strength, xy = _measure_cases()["hand made"]
    f = _filters((33, 65))
    want = _measure_want("hand made", True, True)[0]
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    for k, entry in ((2, (5, len(pts), 0, 0)), (0, (-1, 3, 0, 0)), (len(chains) - 1, (4, 0, 0, 0)), (5, (2 ** 31 - 1, 2 ** 31 - 1, 1, 0))):
        bad = np.array(chains)
        bad[k] = entry
        got = f.chain_measures(up(pts), up(bad), up(strength), up(xy))
        assert got[k].tolist() == (0, 0, 0, -1, 0.0, 0.0, 0.0, 0.0), (k, got[k])
        keep = np.arange(len(chains)) != k
        assert got[keep].tobytes() == f.chain_measures(up(pts), up(chains), up(strength), up(xy))[keep].tobytes()
        assert np.array_equal(got["peak_index"][keep], want["peak_index"][keep])
        with pytest.raises(cv.CvsError) as ei:                                  # the same table on the host is refused
            f.chain_measures(np.array(pts), bad, np.array(strength), np.array(xy))
        assert ei.value.status == L.E_BADARG


# ---- errors ----
def _raw_refine(f, m, theta, pts, n, xy, st, mem):
    ptr = lambda a: None if a is None else C.c_void_p(a if isinstance(a, int) else (a.data_ptr() if torch.is_tensor(a) else a.ctypes.data))
    pm = None if m is None else C.byref(cv.api._plane(m))
    pt = None if theta is None else C.byref(cv.api._plane(theta))
    return L.lib().cvs_chain_refine(f._h, pm, pt, ptr(pts), n, ptr(xy), ptr(st), mem)


def test_refine_errors_leave_the_outputs_untouched():
    shape = (33, 65)
    f = _filters(shape)
    m, theta = (torch.from_numpy(np.array(a)).to(DEV) for a in _case(shape, 11))
    pts = torch.tensor([[1, 1], [2, 2], [64, 32]], dtype=torch.int32, device=DEV)
    xy = torch.full((3, 2), -9.0, device=DEV)
    st = torch.full((3,), -9.0, device=DEV)
    f._bind_stream(m)
    D, H = L.MEM_DEVICE, L.MEM_HOST
    assert _raw_refine(f, m, theta, pts, 0, xy, st, D) == 0                       # nothing to do
    assert _raw_refine(f, m, theta, None, 0, None, None, D) == 0
    assert _raw_refine(f, m, theta, pts, -1, xy, st, D) == L.E_BADARG
    assert _raw_refine(f, m, theta, None, 3, xy, st, D) == L.E_BADARG
    assert _raw_refine(f, m, theta, pts, 3, None, st, D) == L.E_BADARG
    assert _raw_refine(f, None, theta, pts, 3, xy, st, D) == L.E_BADARG
    assert _raw_refine(f, m, theta, pts, 3, xy, st, 7) == L.E_BADARG
    assert _raw_refine(f, m, theta, pts.data_ptr() + 2, 2, xy, st, D) == L.E_BADARG          # not aligned to 4 bytes
    assert _raw_refine(f, m, theta, pts, 3, xy.data_ptr() + 1, st, D) == L.E_BADARG
    assert _raw_refine(f, m, theta, pts, 3, xy, st.data_ptr() + 2, D) == L.E_BADARG
    assert _raw_refine(f, m, theta, pts, 3, pts, st, D) == L.E_BADARG                        # xy is points
    assert _raw_refine(f, m, theta, pts, 3, xy, xy, D) == L.E_BADARG                         # strength inside xy
    assert _raw_refine(f, m, theta, pts, 3, xy, xy.data_ptr() + 16, D) == L.E_BADARG
    assert _raw_refine(f, m, theta, pts, 3, m, st, D) == L.E_BADARG                          # xy inside the map
    assert _raw_refine(f, m, theta, pts, 3, xy, m.data_ptr() + 400, D) == L.E_BADARG         # strength inside the map
    assert _raw_refine(f, m[:, :64], theta, pts, 3, xy, st, D) == L.E_SIZE                   # a plane of another size
    assert _raw_refine(f, m, theta[:32], pts, 3, xy, st, D) == L.E_SIZE
    # a host list with a point outside the image is refused before anything is queued; the same list on the device gives NaN
    hp = np.int32([[1, 1], [65, 2], [3, 3]])
    hxy, hst = np.full((3, 2), -9, F32), np.full((3,), -9, F32)
    for p in ((65, 2), (-1, 0), (0, 33), (0, -1)):
        hp[1] = p
        assert _raw_refine(f, _np(m), _np(theta), hp, 3, hxy, hst, H) == L.E_BADARG
    assert (hxy == -9).all() and (hst == -9).all()
    # no orientation state: theta = NULL is a state error; no image size yet: every call is
    plain = cv.SteerableFiltersG2(None)
    plain._bind_stream(m)
    assert _raw_refine(plain, m, theta, pts, 3, xy, st, D) == L.E_STATE
    assert _raw_refine(plain, m, None, pts, 3, xy, st, D) == L.E_STATE
    basis_only = cv.SteerableFiltersG2(torch.zeros(shape, device=DEV), setup_flags=cv.api.SETUP_BASIS)
    basis_only._bind_stream(m)
    assert _raw_refine(basis_only, m, None, pts, 3, xy, st, D) == L.E_STATE
    torch.cuda.synchronize()
    assert bool((xy == -9).all()) and bool((st == -9).all())
    assert _raw_refine(basis_only, m, theta, pts, 3, xy, None, D) == 0                        # explicit theta, no strength: fine
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xy).all()) and bool((st == -9).all())


def test_measure_errors_leave_the_table_untouched():
    pts, chains, strength, xy = _measure_cases()["random 0.15"]
    f = _filters((33, 65))
    dp, dc, ds, dx = (torch.from_numpy(np.array(a)).to(DEV) for a in (pts, chains, strength, xy))
    tab = torch.full((len(chains), 10), -9, dtype=torch.int32, device=DEV)
    f._bind_stream(dp)
    ptr = lambda a: None if a is None else C.c_void_p(a if isinstance(a, int) else (a.data_ptr() if torch.is_tensor(a) else a.ctypes.data))
    call = lambda p, n, c, k, x, s, t, mem: L.lib().cvs_chain_measures(f._h, ptr(p), n, ptr(c), k, ptr(x), ptr(s), ptr(t), mem)
    n, k, D, H = len(pts), len(chains), L.MEM_DEVICE, L.MEM_HOST
    assert call(dp, n, dc, 0, dx, ds, tab, D) == 0 and call(None, 0, None, 0, None, None, None, D) == 0
    assert call(dp, -1, dc, k, dx, ds, tab, D) == L.E_BADARG and call(dp, n, dc, -1, dx, ds, tab, D) == L.E_BADARG
    assert call(None, n, dc, k, dx, ds, tab, D) == L.E_BADARG and call(dp, n, None, k, dx, ds, tab, D) == L.E_BADARG
    assert call(dp, n, dc, k, dx, ds, None, D) == L.E_BADARG and call(dp, n, dc, k, dx, ds, tab, 5) == L.E_BADARG
    assert call(dp, n, dc, k, dx.data_ptr() + 2, ds, tab, D) == L.E_BADARG and call(dp, n, dc, k, dx, ds, tab.data_ptr() + 1, D) == L.E_BADARG
    assert call(dp, n, dc, k, dx, ds, dc, D) == L.E_BADARG and call(dp, n, dc, k, dx, ds, dp, D) == L.E_BADARG       # the table over an input
    ht = np.full((k, 10), -9, np.int32)
    bad = np.array(chains)
    bad[-1, 1] += 1
    assert call(np.array(pts), n, bad, k, np.array(xy), np.array(strength), ht, H) == L.E_BADARG
    bad = np.array(chains)
    bad[0, 0] = -1
    assert call(np.array(pts), n, bad, k, None, None, ht, H) == L.E_BADARG
    torch.cuda.synchronize()
    assert bool((tab == -9).all()) and (ht == -9).all()


# ---- end to end ----
def test_contour_edgels_end_to_end(fish):
    d = torch.from_numpy(fish).to(DEV)
    f = cv.SteerableFiltersG2(d)
    edges = f.pipeline(d)[5]
    hi = float(f.nonmax(edges).max())
    mask = f.contours(d, 0.05 * hi, 0.2 * hi)[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pts, chains, xy, st, tab = f.contour_edgels(mask, edges)
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    t0 = time.perf_counter()
    f.chain_refine(pts, edges)
    torch.cuda.synchronize()
    t_ref = time.perf_counter() - t0
    dev_tab = torch.empty((len(chains), 40), dtype=torch.uint8, device=DEV)
    t0 = time.perf_counter()
    f.chain_measures(pts, chains, strength=st, xy=xy, out=dev_tab)
    torch.cuda.synchronize()
    t_mea = time.perf_counter() - t0
    print("contour_edgels %d x %d: %d chains, %d points; wall clock contour_edgels %.3f ms, chain_refine %.3f ms, chain_measures %.3f ms"
          % (fish.shape[0], fish.shape[1], len(chains), len(pts), 1e3 * t_all, 1e3 * t_ref, 1e3 * t_mea))
    assert xy.is_cuda and st.is_cuda and isinstance(tab, np.ndarray) and len(pts) > 1000 and len(chains) > 20
    P = M.refine_map(edges.cpu().numpy(), *M.directions(f.getDominantOrientationAngle().cpu().numpy()))
    points = pts.cpu().numpy()
    # the mask holds pixels the kernel's thinning kept; a pixel the model's thinning drops (a decision on the last bits of cos / sin) is
    # not a point of the tolerance tier
    kept = P["keep"][points[:, 1], points[:, 0]]
    print("points the model's thinning keeps too: %d of %d" % (int(kept.sum()), len(points)))
    assert kept.sum() >= 0.98 * len(points)
    hxy, hst = xy.cpu().numpy(), st.cpu().numpy()
    _check_tolerance(P, points[kept], hxy[kept], hst[kept], "fish edges")
    assert np.isfinite(hxy).all() and (np.abs(hxy - points) <= 0.5).all()
    want, abs_sum, abs_len = M.measures(points, chains.cpu().numpy(), hst, hxy, return_abs=True)
    _check_measures(tab, want, abs_sum, abs_len, chains.cpu().numpy())
    assert tab.tobytes() == dev_tab.cpu().numpy().tobytes()
    assert (tab["other"] == 0).all() and (tab["peak"] >= 0.05 * hi * 0.999).all()
    # the numpy path end to end
    hp, hc, hx, hs, ht = f.contour_edgels(mask.cpu().numpy(), edges.cpu().numpy())
    assert isinstance(hx, np.ndarray) and np.array_equal(hp, points) and np.array_equal(_bits(hx), _bits(hxy)) and ht.tobytes() == tab.tobytes()


# ---- facade ----
def test_facade_member(tmp_path):
    from helpers import rand_image
    exe = os.path.join(str(tmp_path), "test_refine")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_refine.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    img = rand_image(33, 65, seed=8)
    pts, table = CM.chains((np.random.default_rng(30).random((33, 65)) < 0.3).astype(F32))
    words = [len(table)]
    for s, n, _, _ in table.tolist():
        words += [n] + pts[s:s + n].reshape(-1).tolist()
    src_img, src, dst = (os.path.join(str(tmp_path), n) for n in ("image.f32", "chains.i32", "edgels.f32"))
    np.ascontiguousarray(img, F32).tofile(src_img)
    np.array(words, np.int32).tofile(src)
    r = subprocess.run([exe, src_img, "33", "65", src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refine OK (%d chains, %d points)" % (len(table), len(pts)) in r.stdout, r.stdout
    got = np.fromfile(dst, F32).reshape(-1, 3)
    f = cv.SteerableFiltersG2(img)                                            # the facade's defaults: the same engine, the same bits
    xy, st = f.chain_refine(pts, img)
    assert np.array_equal(_bits(got[:, :2]), _bits(xy)) and np.array_equal(_bits(got[:, 2]), _bits(st))
    assert (xy != pts).any()
