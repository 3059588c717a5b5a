"""GPU test (-m gpu): contour polylines -- cvs_chain_polylines, chain_polylines, contour_polylines and approxContours against the Python model
of polyline_model.py.  Every comparison is exact (np.array_equal on int32): the values are integers and the one floating-point test is fixed
by the contract.  The chain lists come from chains_model.py on the host and are uploaded, so these tests run the polyline kernels alone; one
test runs contour_polylines end to end."""
import ctypes as C
import functools
import os
import re
import subprocess
import time

import numpy as np
import pytest
import torch

import chains_model as CM
import cvsteer_amd as cv
import polyline_model as M
from cvsteer_amd import _lib as L
from test_gpu_components import serpentine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF = float("inf")
T = int(re.search(r"constexpr int kPlWaveMax = (\d+);", open(os.path.join(ROOT, "cvsteer_amd", "csrc", "cvs_polyline.h")).read()).group(1))
EPS = (0.0, 0.5, 1.0, 1.5, INF)
_cache = {}


def _filters():
    """one handle for all calls: the call needs no image size"""
    if "f" not in _cache:
        _cache["f"] = cv.SteerableFiltersG2(None)
    return _cache["f"]


@functools.lru_cache(maxsize=None)
def _random_chains(density):
    mask = (np.random.default_rng(int(100 * density)).random((33, 65)) < density).astype(np.float32)
    pts, table = CM.chains(mask)
    pts.setflags(write=False)
    table.setflags(write=False)
    return pts, table


@functools.lru_cache(maxsize=None)
def _random_want(density, eps):
    return M.polylines(*_random_chains(density), eps)


def _check(pts, table, eps, path, want=None, what=""):
    """chain_polylines on one path against the model: vertices, table and index, exactly"""
    want_v, want_t, want_i = want if want is not None else M.polylines(pts, table, eps)
    f = _filters()
    if path == "device":
        got = f.chain_polylines(torch.from_numpy(np.array(pts)).to(DEV), torch.from_numpy(np.array(table)).to(DEV), eps, return_index=True)
        assert all(g.is_cuda and g.dtype == torch.int32 for g in got)
        v, t, i = (g.cpu().numpy() for g in got)
    else:
        v, t, i = f.chain_polylines(np.array(pts), np.array(table), eps, return_index=True)
        assert all(isinstance(g, np.ndarray) and g.dtype == np.int32 for g in (v, t, i))
    print("polylines %s eps %s %s: %d chains, %d points -> %d vertices (longest chain %d)"
          % (what, eps, path, len(table), len(pts), len(want_v), int(table[:, 1].max()) if len(table) else 0))
    assert v.shape == want_v.shape and t.shape == want_t.shape and i.shape == want_i.shape, (v.shape, want_v.shape, t.shape, want_t.shape)
    assert np.array_equal(t, want_t), int(np.count_nonzero((t != want_t).any(axis=1)))
    assert np.array_equal(i, want_i), int(np.count_nonzero(i != want_i))
    assert np.array_equal(v, want_v), int(np.count_nonzero((v != want_v).any(axis=1)))
    assert np.array_equal(v, np.asarray(pts)[i])                                           # index maps the vertices back to the points
    return v, t, i


@pytest.mark.parametrize("path", ["device", "host"])
@pytest.mark.parametrize("density", [0.15, 0.3, 0.5])
def test_random_masks(density, path):
    pts, table = _random_chains(density)
    for eps in EPS:
        _check(pts, table, eps, path, _random_want(density, eps), "random %.2f" % density)


def _mask_chains(mask):
    pts, table = CM.chains(mask)
    return pts, table


def test_serpentine_reaches_the_workgroup_kernel():
    pts, table = _mask_chains((serpentine(64) > 0).astype(np.float32))
    assert table.tolist() == [[0, 1037, 0, 0]] and 1037 > 1024 >= T      # one open chain, beyond any allowed kPlWaveMax
    for eps in (0.0, 1.0, INF):
        v, t, i = _check(pts, table, eps, "device", what="serpentine 64")
    assert len(v) == 2
    _check(pts, table, 1.0, "host", what="serpentine 64")


def test_ring():
    y, x = np.mgrid[0:64, 0:64]
    d = np.hypot(y - 32, x - 32)
    pts, table = _mask_chains(((d >= 20) & (d < 21)).astype(np.float32))
    assert len(pts) > 64
    for eps in (0.5, 1.0, 3.0):
        _check(pts, table, eps, "device", what="ring")


def _zigzag(n, seed):
    """n points walking right with a random height: splits land anywhere"""
    rng = np.random.default_rng(seed)
    return np.stack([np.arange(n), rng.integers(0, 9, n)], axis=1).astype(np.int32)


def _pack(lists, flags=None):
    pts = np.concatenate(lists).astype(np.int32).reshape(-1, 2)
    table, start = [], 0
    for k, p in enumerate(lists):
        table.append((start, len(p), 0 if flags is None else flags[k], 0))
        start += len(p)
    return pts, np.array(table, np.int32).reshape(-1, 4)


LENGTHS = (1, 2, 3, 63, 64, 65, 66, T - 1, T, T + 1, 4 * T + 3)


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_zigzag_lengths_around_the_wave_limit(order):
    lists = [_zigzag(n, seed=n) for n in (LENGTHS if order == "ascending" else LENGTHS[::-1])]
    pts, table = _pack(lists)
    for eps in (1.5, 3.0):
        v, t, i = _check(pts, table, eps, "device", what="zigzag " + order)
    assert t[:, 1].min() >= 1
    _check(pts, table, 1.5, "host", what="zigzag " + order)
    # the same chains as cycles: the virtual last point
    closed = [CM.CLOSED] * len(lists)
    _check(*_pack(lists, closed), 1.5, "device", what="closed zigzag " + order)


def test_many_isolated_points_with_long_chains_between():
    i = np.arange(4096)
    lists = [np.array([[3 * k, 7 * (k % 50)]], np.int32) for k in i]
    for at, n in ((100, 300), (1500, 2 * T + 77), (4000, 4 * T + 1)):
        s = np.arange(n)
        lists.insert(at, np.stack([s, np.rint(20 * np.sin(s / 15.0) + 3 * np.cos(s / 2.0)).astype(np.int64)], axis=1).astype(np.int32))
    pts, table = _pack(lists)
    assert len(table) == 4099 and int((table[:, 1] > T).sum()) == 3
    v, t, i = _check(pts, table, 1.0, "device", what="isolated + long")
    assert int((t[:, 1] == 1).sum()) == 4096
    _check(pts, table, 1.0, "host", what="isolated + long")


def test_no_chains():
    for path in ("device", "host"):
        v, t, i = _check(np.zeros((0, 2), np.int32), np.zeros((0, 4), np.int32), 1.0, path, what="empty")
        assert v.shape == (0, 2) and t.shape == (0, 4) and i.shape == (0,)
    # points without chains
    _check(np.zeros((5, 2), np.int32), np.zeros((0, 4), np.int32), 1.0, "device", what="no chains")


def test_closed_chain_and_loop_through_a_junction():
    ring = [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (3, 2), (3, 3), (2, 3), (1, 3), (0, 3), (0, 2), (0, 1)]
    loop = [(2, 2), (3, 2), (4, 2), (4, 3), (4, 4), (3, 4), (2, 4), (2, 3), (2, 2)]
    both = CM.HEAD_JUNCTION | CM.TAIL_JUNCTION
    pts, table = _pack([np.int32(ring), np.int32(loop), np.int32(ring[:2]), np.int32(ring)], [CM.CLOSED, both, CM.CLOSED, 0])
    for path in ("device", "host"):
        v, t, i = _check(pts, table, 1.0, path, what="ring + loop")
        assert i.tolist() == [0, 3, 6, 9, 12, 14, 16, 18, 20, 21, 22, 23, 26, 29, 32, 34]
        assert t.tolist() == [[0, 4, CM.CLOSED, 0], [4, 5, both, 0], [9, 2, CM.CLOSED, 0], [11, 5, 0, 0]]
        v, t, i = _check(pts, table, INF, path, what="ring + loop")
        assert i.tolist() == [0, 12, 20, 21, 22, 23, 34]


def test_tent_at_the_tolerance_and_just_below_it():
    tent = np.int32([(0, 2), (0, 1), (0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 1), (4, 2)])
    table = np.int32([[0, 9, 0, 0]])
    below = float(np.nextafter(np.float32(2.0), np.float32(0.0)))
    for path in ("device", "host"):
        assert _check(tent, table, 2.0, path, what="tent")[2].tolist() == [0, 8]
        assert _check(tent, table, below, path, what="tent")[2].tolist() == [0, 2, 8]
        assert _check(tent[2:7].copy(), np.int32([[0, 5, 0, 0]]), 0.0, path, what="run")[2].tolist() == [0, 4]


def _raw(f, pts, table, eps, vtx, idx, pol, cap, mem):
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr() if torch.is_tensor(a) else a.ctypes.data)
    n = C.c_int(-7)
    rc = L.lib().cvs_chain_polylines(f._h, ptr(pts), len(pts), ptr(table), len(table), eps, ptr(vtx), cap, ptr(idx), ptr(pol), mem, C.byref(n))
    return rc, n.value


def test_capacity_errors_and_run_to_run_identity():
    f = _filters()
    pts, table = _random_chains(0.3)
    want_v, want_t, want_i = _random_want(0.3, 1.0)
    nv, npts, nch = len(want_v), len(pts), len(table)
    dp, dt = torch.from_numpy(np.array(pts)).to(DEV), torch.from_numpy(np.array(table)).to(DEV)
    f._bind_stream(dp)
    # sizing call, then one entry too few: CVS_E_SIZE, the count set, every sentinel in place
    assert _raw(f, dp, dt, 1.0, None, None, None, 0, L.MEM_DEVICE) == (L.E_SIZE, nv)
    vtx = torch.full((npts, 2), -9, dtype=torch.int32, device=DEV)
    idx = torch.full((npts,), -9, dtype=torch.int32, device=DEV)
    pol = torch.full((nch, 4), -9, dtype=torch.int32, device=DEV)
    assert _raw(f, dp, dt, 1.0, vtx, idx, pol, nv - 1, L.MEM_DEVICE) == (L.E_SIZE, nv)
    torch.cuda.synchronize()
    assert bool((vtx == -9).all()) and bool((idx == -9).all()) and bool((pol == -9).all())
    hv, hi, hp = np.full((npts, 2), -9, np.int32), np.full((npts,), -9, np.int32), np.full((nch, 4), -9, np.int32)
    assert _raw(f, np.array(pts), np.array(table), 1.0, hv, hi, hp, nv - 1, L.MEM_HOST) == (L.E_SIZE, nv)
    assert (hv == -9).all() and (hi == -9).all() and (hp == -9).all()
    # an exact capacity: the lists, and nothing behind them
    assert _raw(f, dp, dt, 1.0, vtx, idx, pol, nv, L.MEM_DEVICE) == (0, nv)
    assert np.array_equal(vtx[:nv].cpu().numpy(), want_v) and np.array_equal(idx[:nv].cpu().numpy(), want_i)
    assert np.array_equal(pol.cpu().numpy(), want_t) and bool((vtx[nv:] == -9).all()) and bool((idx[nv:] == -9).all())
    assert _raw(f, np.array(pts), np.array(table), 1.0, hv, None, hp, nv, L.MEM_HOST) == (0, nv)            # no index
    assert np.array_equal(hv[:nv], want_v) and np.array_equal(hp, want_t) and (hv[nv:] == -9).all() and (hi == -9).all()
    # rejected arguments: nothing written, the count untouched
    vtx.fill_(-9), idx.fill_(-9), pol.fill_(-9)
    for eps in (float("nan"), -1.0, -INF):
        assert _raw(f, dp, dt, eps, vtx, idx, pol, npts, L.MEM_DEVICE) == (L.E_BADARG, -7)
    assert _raw(f, dp, dt, 1.0, vtx, idx, pol, npts, 7) == (L.E_BADARG, -7)
    assert _raw(f, dp, dt, 1.0, None, idx, pol, npts, L.MEM_DEVICE) == (L.E_BADARG, -7)                       # a capacity without vertices
    assert _raw(f, dp, dt, 1.0, vtx, idx, None, npts, L.MEM_DEVICE) == (L.E_BADARG, -7)                       # ... without the table
    assert _raw(f, dp, dt, 1.0, vtx, idx, pol, -1, L.MEM_DEVICE) == (L.E_BADARG, -7)
    bad = np.array(table)
    bad[-1, 1] += 1                                                                                           # start + length > n_points
    assert _raw(f, np.array(pts), bad, 1.0, hv, hi, hp, npts, L.MEM_HOST) == (L.E_BADARG, -7)
    bad = np.array(table)
    bad[0, 1] = 0
    assert _raw(f, np.array(pts), bad, 1.0, hv, hi, hp, npts, L.MEM_HOST) == (L.E_BADARG, -7)
    torch.cuda.synchronize()
    assert bool((vtx == -9).all()) and bool((idx == -9).all()) and bool((pol == -9).all())
    # two calls: identical bytes
    a = f.chain_polylines(dp, dt, 1.0, return_index=True)
    b = f.chain_polylines(dp, dt, 1.0, return_index=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a[0].cpu().numpy().tobytes() == want_v.tobytes() and a[1].cpu().numpy().tobytes() == want_t.tobytes()
    assert len(f.chain_polylines(dp, dt, 1.0)) == 2


def test_an_array_that_is_not_aligned_to_4_bytes_is_refused():
    """each of the five arrays in turn two bytes off, on both paths: CVS_E_BADARG, the count and every output untouched (one entry fewer
    is passed than the arrays hold, so that nothing could be read behind them)"""
    f = _filters()
    pts, table = _random_chains(0.3)
    npts, nch = len(pts), len(table)
    dev = [torch.from_numpy(np.array(pts)).to(DEV), torch.from_numpy(np.array(table)).to(DEV),
           torch.full((npts, 2), -9, dtype=torch.int32, device=DEV), torch.full((npts,), -9, dtype=torch.int32, device=DEV),
           torch.full((nch, 4), -9, dtype=torch.int32, device=DEV)]
    host = [np.array(pts), np.array(table), np.full((npts, 2), -9, np.int32), np.full((npts,), -9, np.int32), np.full((nch, 4), -9, np.int32)]
    f._bind_stream(dev[0])
    for arrays, mem in ((dev, L.MEM_DEVICE), (host, L.MEM_HOST)):
        for k in range(5):
            p = [C.c_void_p((a.data_ptr() if torch.is_tensor(a) else a.ctypes.data) + (2 if j == k else 0)) for j, a in enumerate(arrays)]
            n = C.c_int(-7)
            rc = L.lib().cvs_chain_polylines(f._h, p[0], npts - 1, p[1], nch - 1, 1.0, p[2], npts - 1, p[3], p[4], mem, C.byref(n))
            assert (rc, n.value) == (L.E_BADARG, -7), (mem, k)
            assert b"not aligned to 4 bytes" in L.lib().cvs_last_error(f._h), (mem, k)
    torch.cuda.synchronize()
    assert all(bool((a == -9).all()) for a in dev[2:]) and all((a == -9).all() for a in host[2:])


def test_capture_is_refused_and_the_handle_works_afterwards():
    f = cv.SteerableFiltersG2(None)
    pts, table = _random_chains(0.15)
    dp, dt = torch.from_numpy(np.array(pts)).to(DEV), torch.from_numpy(np.array(table)).to(DEV)
    vtx = torch.full((len(pts), 2), -9, dtype=torch.int32, device=DEV)
    pol = torch.full((len(table), 4), -9, dtype=torch.int32, device=DEV)
    good = f.chain_polylines(dp, dt, 1.0)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    junk = torch.zeros(8, device=DEV)
    with torch.cuda.stream(side):
        f.chain_polylines(dp, dt, 1.0)               # the handle moves to the side stream outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            junk.fill_(1.0)
            rc, n = _raw(f, dp, dt, 1.0, vtx, None, pol, len(pts), L.MEM_DEVICE)
    assert (rc, n) == (L.E_UNSUPPORTED, -7)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert bool((vtx == -9).all()) and bool((pol == -9).all())
    again = f.chain_polylines(dp, dt, 1.0)
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])
    assert np.array_equal(good[0].cpu().numpy(), _random_want(0.15, 1.0)[0])


def test_contour_polylines_end_to_end():
    mask = (np.random.default_rng(30).random((33, 65)) < 0.3).astype(np.float32)
    want_v, want_t, want_i = M.polylines(*CM.chains(mask), 1.0)
    for kind in (cv.SteerableFiltersG2, cv.SteerableFiltersG4):
        f = kind(None)
        f.setup(torch.zeros(mask.shape, device=DEV))
        v, t, i = f.contour_polylines(torch.from_numpy(mask).to(DEV), 1.0, return_index=True)
        assert np.array_equal(t.cpu().numpy(), want_t) and np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(v.cpu().numpy(), want_v)
    hv, ht = f.contour_polylines(mask, 1.0)
    assert isinstance(hv, np.ndarray) and np.array_equal(hv, want_v) and np.array_equal(ht, want_t)


def test_facade_members(tmp_path):
    exe = os.path.join(str(tmp_path), "test_polylines")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_polylines.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    pts, table = _random_chains(0.3)
    words = [len(table)]
    for s, n, fl, _ in table.tolist():
        words += [n, fl] + pts[s:s + n].reshape(-1).tolist()
    src, dst = os.path.join(str(tmp_path), "chains.i32"), os.path.join(str(tmp_path), "polylines.i32")
    np.array(words, np.int32).tofile(src)
    r = subprocess.run([exe, src, dst, "1.0"], capture_output=True, text=True, timeout=120)
    want_v, want_t, _ = _random_want(0.3, 1.0)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "polylines OK (%d chains, %d vertices)" % (len(table), len(want_v)) in r.stdout, r.stdout
    got = np.fromfile(dst, np.int32).tolist()
    want = [len(want_v)]
    for s, n, _, _ in want_t.tolist():
        want += [n] + want_v[s:s + n].reshape(-1).tolist()
    assert got == want


def test_polyline_times_print():
    """wall clock around the (synchronising) call, printed; no threshold"""
    f = _filters()
    s = np.arange(200000)
    wave = np.stack([s, np.rint(40 * np.sin(s / 60.0)).astype(np.int64)], axis=1).astype(np.int32)
    cases = {"one chain of 200000 points": _pack([wave]), "random mask 33 x 65": _random_chains(0.3)}
    for name, (pts, table) in cases.items():
        dp, dt = torch.from_numpy(np.array(pts)).to(DEV), torch.from_numpy(np.array(table)).to(DEV)
        f.chain_polylines(dp, dt, 1.0)   # warm: scratch allocated, code loaded
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            v, t = f.chain_polylines(dp, dt, 1.0)
            ts.append(time.perf_counter() - t0)
        print("chain_polylines %s: %.3f ms (%d chains, %d points -> %d vertices)" % (name, 1e3 * float(np.median(ts)), len(t), len(pts), len(v)))
        assert 2 <= len(v) <= len(pts) and int(t[:, 1].sum()) == len(v)
