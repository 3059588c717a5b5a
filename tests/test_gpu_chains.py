"""GPU test (-m gpu): contour chains -- cvs_contour_chains, contour_chains and traceContours against the Python model of chains_model.py.
Every comparison is exact (np.array_equal on int32): all arithmetic is integer, there is nothing to tolerate."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest
import torch

import chains_model as M
import cvsteer_amd as cv
from cvsteer_amd import _lib as L
from test_gpu_components import double_spiral, serpentine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
_hdr = open(os.path.join(ROOT, "cvsteer_amd", "csrc", "cvs_components.h")).read()
TILE_W = int(re.search(r"constexpr int kCcTileW = (\d+);", _hdr).group(1))
TILE_H = int(re.search(r"constexpr int kCcTileH = (\d+);", _hdr).group(1))
_handles = {}


def _handle(shape, kind="g2"):
    """a handle whose image size is `shape` (the call reads no state: any image will do)"""
    key = (tuple(shape), kind)
    if key not in _handles:
        f = cv.SteerableFiltersG2(None) if kind == "g2" else cv.SteerableFiltersG4(None)
        f.setup(torch.zeros(tuple(shape), device=DEV))
        _handles[key] = f
    return _handles[key]


def _check(mask, f=None, what=""):
    mask = np.ascontiguousarray(mask)
    f = f or _handle(mask.shape)
    pts, table = f.contour_chains(torch.from_numpy(mask).to(DEV))
    want_p, want_t = M.chains(mask)
    assert pts.dtype == torch.int32 and table.dtype == torch.int32 and pts.is_cuda and table.is_cuda
    print("chains %s %s: %d chains, %d points" % (mask.shape, what, len(want_t), len(want_p)))
    assert tuple(pts.shape) == want_p.shape and tuple(table.shape) == want_t.shape, (tuple(pts.shape), want_p.shape, tuple(table.shape), want_t.shape)
    gt, gp = table.cpu().numpy(), pts.cpu().numpy()
    assert np.array_equal(gt, want_t), int(np.count_nonzero((gt != want_t).any(axis=1)))
    assert np.array_equal(gp, want_p), int(np.count_nonzero((gp != want_p).any(axis=1)))
    return gp, gt


def _random_mask(shape, density, seed=7):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.float32)


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (29, 1), (2, 2), (3, 257), (67, 300), (517, 731)])
def test_chains_random(shape):
    for density in ((0.03, 0.1) if shape == (517, 731) else (0.03, 0.1, 0.3, 0.6)):
        _check(_random_mask(shape, density, seed=int(100 * density) + shape[1]), what="density %.2f" % density)


def test_chains_structured():
    shape = (33, 130)
    f = _handle(shape)
    rows, cols = shape
    pts, table = _check(np.ones(shape, np.float32), f, "all foreground")       # every pixel but the four corners is a node
    assert (table[:, 1] <= 3).all() and int((table[:, 1] == 3).sum()) == 4
    pts, table = _check(np.zeros(shape, np.float32), f, "all background")
    assert pts.shape == (0, 2) and table.shape == (0, 4)
    r, c = np.mgrid[0:rows, 0:cols]
    _check(((r + c) % 2 == 0).astype(np.float32), f, "checkerboard")
    pts, table = _check(((r % 2 == 0) & (c % 2 == 0)).astype(np.float32), f, "isolated pixels")
    assert len(table) == ((rows + 1) // 2) * ((cols + 1) // 2) and (table[:, 1] == 1).all() and (table[:, 2] == 0).all()


def _hand_cases():
    ring = np.zeros((5, 5), np.float32)
    ring[0, :] = ring[4, :] = ring[:, 0] = ring[:, 4] = 1
    eight = ring.copy()
    eight[2, :] = 1
    tee = np.float32([[1, 1, 1, 1, 1], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0]])
    return {"block": np.ones((2, 2), np.float32), "ring": ring, "eight": eight, "tee": tee, "pixel": np.ones((1, 1), np.float32)}


def test_hand_cases_across_a_tile_corner():
    shape = (2 * TILE_H + 3, 2 * TILE_W + 3)
    f = _handle(shape)
    for name, case in _hand_cases().items():
        for y0 in (TILE_H - 1, TILE_H - 2):
            for x0 in (TILE_W - 1, TILE_W - 2):
                m = np.zeros(shape, np.float32)
                m[y0:y0 + case.shape[0], x0:x0 + case.shape[1]] = case
                pts, table = _check(m, f, name)
                if name in ("block", "ring"):
                    assert table.tolist() == [[0, int(case.sum()), M.CLOSED, 0]] and pts[0].tolist() == [x0, y0] and pts[1].tolist() == [x0 + 1, y0]
                if name == "eight":
                    assert len(table) == 3 and (table[:, 2] == (M.HEAD_JUNCTION | M.TAIL_JUNCTION)).all()


def test_serpentine_is_one_open_chain():
    m = (serpentine(1024) > 0).astype(np.float32)
    pts, table = _check(m, what="serpentine")
    assert table.tolist() == [[0, int(m.sum()), 0, 0]]


def test_double_spiral():
    _check(double_spiral(), what="double spiral")


def test_long_ring_is_cut_at_its_root_and_a_spur_moves_the_cut():
    shape = (600, 1500)
    f = _handle(shape)
    ring = np.zeros(shape, np.float32)
    ring[1, 1:1499] = ring[598, 1:1499] = ring[1:599, 1] = ring[1:599, 1498] = 1
    n = int(ring.sum())
    assert n > 4096
    pts, table = _check(ring, f, "ring")
    assert table.tolist() == [[0, n, M.CLOSED, 0]] and pts[0].tolist() == [1, 1] and pts[1].tolist() == [2, 1]
    spur = ring.copy()
    spur[300, 2:40] = 1   # the smallest pixel still has degree 2, but the component is no cycle: the chains start at the junction
    pts, table = _check(spur, f, "ring with a spur")
    assert len(table) == 2 and not (table[:, 2] & M.CLOSED).any()
    assert pts[0].tolist() == [1, 300] and sorted(table[:, 1].tolist()) == [39, n + 1]


def _thinned_masks():
    if "thinned" not in _handles:
        _handles["thinned"] = _make_thinned_masks()
    return _handles["thinned"]


def _make_thinned_masks():
    rows, cols = 240, 320
    rng = np.random.default_rng(12)
    y, x = np.mgrid[0:rows, 0:cols]
    img = np.zeros((rows, cols), np.float32)
    for cy, cx, r in ((60, 80, 30), (150, 220, 45), (190, 70, 20)):
        img[(y - cy) ** 2 + (x - cx) ** 2 < r * r] = 200
    img[100:108, 20:300] = 120
    img[20:220, 150:155] = 60
    img += rng.normal(0, 4, img.shape).astype(np.float32)
    f = cv.SteerableFiltersG2(torch.from_numpy(img).to(DEV))
    d = torch.from_numpy(img).to(DEV)
    thin = f.nonmax(f.pipeline(d)[5:8])
    hi = float(max(float(t.max()) for t in thin))
    return f, f.contours(d, 0.05 * hi, 0.2 * hi)


def test_chains_of_a_real_thinned_map():
    f, masks = _thinned_masks()
    for name, m in zip(("edges", "dark", "bright"), masks):
        assert m.dtype == torch.uint8 and bool(m.any())
        want_p, want_t = M.chains(m.cpu().numpy())
        pts, table = f.contour_chains(m)
        print("thinned %s: %d chains, %d points" % (name, len(want_t), len(want_p)))
        assert np.array_equal(table.cpu().numpy(), want_t) and np.array_equal(pts.cpu().numpy(), want_p)


@pytest.mark.parametrize("kind", ["g2", "g4"])
def test_mask_kinds_memory_and_pitch(kind):
    rows, cols = 150, 203
    f = _handle((rows, cols), kind)
    rng = np.random.default_rng(3)
    v = _random_mask((rows, cols), 0.25, seed=5) * rng.random((rows, cols), dtype=np.float32)
    v.flat[rng.integers(0, v.size, 200)] = np.nan
    v.flat[rng.integers(0, v.size, 200)] = -1.0
    v.flat[rng.integers(0, v.size, 200)] = np.inf
    want_p, want_t = M.chains(v)
    same = lambda got: np.array_equal(np.asarray(got[0].cpu() if torch.is_tensor(got[0]) else got[0]), want_p) and \
        np.array_equal(np.asarray(got[1].cpu() if torch.is_tensor(got[1]) else got[1]), want_t)
    assert same(f.contour_chains(torch.from_numpy(v).to(DEV)))                 # f32, device
    hp, ht = f.contour_chains(v)                                               # f32, host: numpy in, numpy out
    assert isinstance(hp, np.ndarray) and isinstance(ht, np.ndarray) and hp.dtype == np.int32 and ht.dtype == np.int32 and same((hp, ht))
    b = np.where(M.foreground(v), rng.integers(1, 256, v.shape), 0).astype(np.uint8)
    assert same(f.contour_chains(torch.from_numpy(b).to(DEV)))                 # u8, device
    assert same(f.contour_chains(b))                                           # u8, host
    wide = torch.full((rows, cols + 9), float("nan"), device=DEV)             # pitched views
    wide[:, 3:3 + cols] = torch.from_numpy(v).to(DEV)
    assert same(f.contour_chains(wide[:, 3:3 + cols]))
    wide_b = torch.full((rows, cols + 11), 255, dtype=torch.uint8, device=DEV)
    wide_b[:, 2:2 + cols] = torch.from_numpy(b).to(DEV)
    assert same(f.contour_chains(wide_b[:, 2:2 + cols]))
    hwide = np.full((rows, cols + 4), 1.0, np.float32)
    hwide[:, 2:2 + cols] = v
    assert same(f.contour_chains(hwide[:, 2:2 + cols]))


def test_capacity_and_run_to_run_identity():
    shape = (67, 300)
    f = _handle(shape)
    m = torch.from_numpy(_random_mask(shape, 0.3, seed=21)).to(DEV)
    want_p, want_t = M.chains(m.cpu().numpy())
    npts, nch = len(want_p), len(want_t)
    pm = cv.api._plane(m)
    lib = L.lib()
    n, k = C.c_int(-1), C.c_int(-1)
    assert lib.cvs_contour_chains(f._h, C.byref(pm), None, 0, None, 0, L.MEM_DEVICE, C.byref(n), C.byref(k)) == L.E_SIZE
    assert (n.value, k.value) == (npts, nch)
    pts = torch.full((npts + 1, 2), -9, dtype=torch.int32, device=DEV)
    tab = torch.full((nch + 1, 4), -9, dtype=torch.int32, device=DEV)
    for cap_p, cap_c in ((npts - 1, nch), (npts, nch - 1)):
        n, k = C.c_int(-1), C.c_int(-1)
        rc = lib.cvs_contour_chains(f._h, C.byref(pm), C.c_void_p(pts.data_ptr()), cap_p, C.c_void_p(tab.data_ptr()), cap_c, L.MEM_DEVICE,
                                    C.byref(n), C.byref(k))
        torch.cuda.synchronize()
        assert rc == L.E_SIZE and (n.value, k.value) == (npts, nch) and bool((pts == -9).all()) and bool((tab == -9).all())
    rc = lib.cvs_contour_chains(f._h, C.byref(pm), C.c_void_p(pts.data_ptr()), npts, C.c_void_p(tab.data_ptr()), nch, L.MEM_DEVICE,
                                C.byref(n), C.byref(k))
    assert rc == 0 and (n.value, k.value) == (npts, nch)
    assert np.array_equal(pts[:npts].cpu().numpy(), want_p) and np.array_equal(tab[:nch].cpu().numpy(), want_t)
    assert bool((pts[npts:] == -9).all()) and bool((tab[nch:] == -9).all())      # nothing beyond the counts
    # host arrays through the C ABI, guard entries behind the lists
    hp, ht = np.full((npts + 1, 2), -9, np.int32), np.full((nch + 1, 4), -9, np.int32)
    rc = lib.cvs_contour_chains(f._h, C.byref(pm), C.c_void_p(hp.ctypes.data), npts, C.c_void_p(ht.ctypes.data), nch, L.MEM_HOST,
                                C.byref(n), C.byref(k))
    assert rc == 0 and np.array_equal(hp[:npts], want_p) and np.array_equal(ht[:nch], want_t) and (hp[npts:] == -9).all() and (ht[nch:] == -9).all()
    # two calls: identical bytes
    a = f.contour_chains(m)
    b = f.contour_chains(m)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].cpu().numpy().tobytes() == want_p.tobytes() and a[1].cpu().numpy().tobytes() == want_t.tobytes()


def test_errors_and_capture():
    rows, cols = 64, 96
    f = _handle((rows, cols))
    lib = L.lib()
    one = lambda t: C.byref(cv.api._plane(t))
    mask = (torch.rand(rows, cols, device=DEV) < 0.3).float()
    small = torch.rand(rows - 1, cols, device=DEV)
    lab = torch.zeros((rows, cols), dtype=torch.int32, device=DEV)
    pts = torch.full((4 * rows * cols, 2), -9, dtype=torch.int32, device=DEV)
    tab = torch.full((4 * rows * cols, 4), -9, dtype=torch.int32, device=DEV)
    pp, pt, cap = C.c_void_p(pts.data_ptr()), C.c_void_p(tab.data_ptr()), 4 * rows * cols
    n, k = C.c_int(-1), C.c_int(-1)
    call = lambda *a: lib.cvs_contour_chains(*a)
    assert call(f._h, None, pp, cap, pt, cap, L.MEM_DEVICE, C.byref(n), C.byref(k)) == L.E_BADARG
    assert call(f._h, one(mask), pp, cap, pt, cap, L.MEM_DEVICE, None, C.byref(k)) == L.E_BADARG
    assert call(f._h, one(mask), pp, cap, pt, cap, L.MEM_DEVICE, C.byref(n), None) == L.E_BADARG
    assert call(f._h, one(mask), None, 5, pt, cap, L.MEM_DEVICE, C.byref(n), C.byref(k)) == L.E_BADARG       # NULL with a capacity
    assert call(f._h, one(mask), pp, cap, None, 5, L.MEM_DEVICE, C.byref(n), C.byref(k)) == L.E_BADARG
    assert call(f._h, one(mask), pp, -1, pt, cap, L.MEM_DEVICE, C.byref(n), C.byref(k)) == L.E_BADARG        # negative capacities
    assert call(f._h, one(mask), pp, cap, pt, -1, L.MEM_DEVICE, C.byref(n), C.byref(k)) == L.E_BADARG
    assert call(f._h, one(mask), pp, cap, pt, cap, 7, C.byref(n), C.byref(k)) == L.E_BADARG                   # mem
    assert call(f._h, one(lab), pp, cap, pt, cap, L.MEM_DEVICE, C.byref(n), C.byref(k)) == L.E_BADARG         # an S32 plane is no mask
    assert call(f._h, one(small), pp, cap, pt, cap, L.MEM_DEVICE, C.byref(n), C.byref(k)) == L.E_SIZE
    fresh = cv.SteerableFiltersG2(None)
    assert call(fresh._h, one(mask), pp, cap, pt, cap, L.MEM_DEVICE, C.byref(n), C.byref(k)) == L.E_STATE     # no setup
    torch.cuda.synchronize()
    assert (n.value, k.value) == (-1, -1) and bool((pts == -9).all()) and bool((tab == -9).all())
    # capture: refused, and the handle works afterwards
    good = f.contour_chains(mask)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    junk = torch.zeros(8, device=DEV)
    with torch.cuda.stream(side):
        f.contour_chains(mask)                   # the handle moves to the side stream outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            junk.fill_(1.0)
            rc = call(f._h, one(mask), pp, cap, pt, cap, L.MEM_DEVICE, C.byref(n), C.byref(k))
    assert rc == L.E_UNSUPPORTED
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert (n.value, k.value) == (-1, -1) and bool((pts == -9).all()) and bool((tab == -9).all())
    again = f.contour_chains(mask)
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])
    want_p, want_t = M.chains(mask.cpu().numpy())
    assert np.array_equal(good[0].cpu().numpy(), want_p) and np.array_equal(good[1].cpu().numpy(), want_t)


def test_facade_members(tmp_path):
    exe = os.path.join(str(tmp_path), "test_chains")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_chains.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    mask = _random_mask((97, 141), 0.2, seed=4) * 255.0
    mask[40:60, 30:50] = 0                                    # a clearing ...
    mask[45:50, 35:40] = _hand_cases()["eight"] * 255.0       # ... with a figure eight in it
    raw = os.path.join(str(tmp_path), "mask.f32")
    mask.astype(np.float32).tofile(raw)
    r = subprocess.run([exe, raw, str(mask.shape[0]), str(mask.shape[1])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want_p, want_t = M.chains(mask.astype(np.float32))
    assert "chains OK (%d chains, %d points)" % (len(want_t), len(want_p)) in r.stdout, r.stdout


def test_chain_times_print():
    """wall clock around the (synchronising) call, printed; no threshold"""
    v = torch.from_numpy((serpentine(1024) > 0).astype(np.float32)).to(DEV)
    f = _handle((1024, 1024))
    ft, masks = _thinned_masks()
    for name, h, m in (("serpentine 1024^2", f, v), ("thinned edges 240 x 320", ft, masks[0])):
        h.contour_chains(m)   # warm: scratch allocated, code loaded
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            pts, table = h.contour_chains(m)
            ts.append(time.perf_counter() - t0)
        print("contour_chains %s: %.3f ms (%d chains, %d points)" % (name, 1e3 * float(np.median(ts)), len(table), len(pts)))
        assert len(pts) > 0
