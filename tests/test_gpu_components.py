"""GPU test (-m gpu): contour components -- cvs_label, cvs_component_stats, cvs_contour_prune and cvs_contour_points against the scipy /
numpy models of components_model.py.  Every comparison is exact (np.array_equal on int32 / uint8 / the bit patterns of `peak`): all
arithmetic is integer or a copy, there is nothing to tolerate."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest
import torch

import components_model as M
import cvsteer_amd as cv
from cvsteer_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
_hdr = open(os.path.join(ROOT, "cvsteer_amd", "csrc", "cvs_components.h")).read()
TILE_W = int(re.search(r"constexpr int kCcTileW = (\d+);", _hdr).group(1))
TILE_H = int(re.search(r"constexpr int kCcTileH = (\d+);", _hdr).group(1))
SHAPES = [(1, 1), (1, 37), (29, 1), (2, 2), (3, 257), (517, 731), (1080, 1920), (4096, 4096)]
_handles = {}


def _handle(shape, kind="g2"):
    """a handle whose image size is `shape` (the component calls read no state: any image will do)"""
    key = (tuple(shape), kind)
    if key not in _handles:
        f = cv.SteerableFiltersG2(None) if kind == "g2" else cv.SteerableFiltersG4(None)
        f.setup(torch.zeros(tuple(shape), device=DEV))
        _handles[key] = f
    return _handles[key]


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _random_mask(shape, density, seed=7):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.float32)


def _check_label(mask, f=None, what=""):
    mask = np.ascontiguousarray(mask)
    f = f or _handle(mask.shape)
    got, n = f.label(torch.from_numpy(mask).to(DEV))
    want, wn = M.label(mask)
    assert got.dtype == torch.int32
    print("label %s %s: %d components" % (mask.shape, what, n))
    assert n == wn, (n, wn)
    g = got.cpu().numpy()
    assert np.array_equal(g, want), int(np.count_nonzero(g != want))
    return got, n


def serpentine(n=1024):
    """the one-pixel path of test_hysteresis_serpentine"""
    v = np.zeros((n, n), np.float32)
    for r in range(1, n - 1, 4):
        v[r, 1:n - 1] = 0.5
        turn = n - 2 if (r // 4) % 2 == 0 else 1
        if r + 4 < n - 1:
            v[r + 1:r + 4, turn] = 0.5
    v[1, 1] = 1.0
    return v


def double_spiral(n=513, pitch=8.0):
    """two one-pixel Archimedean spirals wound into each other, half a pitch apart: two components, each as long as a contour gets"""
    m = np.zeros((n, n), np.float32)
    c = n // 2
    t = np.linspace(np.pi, (c - 2) / pitch * 2 * np.pi, 400000)
    r = pitch * t / (2 * np.pi)
    for phase in (0.0, np.pi):
        m[np.rint(c + r * np.sin(t + phase)).astype(int), np.rint(c + r * np.cos(t + phase)).astype(int)] = 1
    return m


@pytest.mark.parametrize("shape", SHAPES)
def test_label_random(shape):
    for density in (0.2, 0.3, 0.45, 0.6):
        _check_label(_random_mask(shape, density), what="density %.2f" % density)


@pytest.mark.parametrize("shape", [(1, 1), (3, 257), (517, 731), (1080, 1920)])
def test_label_structured(shape):
    rows, cols = shape
    f = _handle(shape)
    got, n = _check_label(np.ones(shape, np.float32), f, "all foreground")
    assert n == 1
    got, n = _check_label(np.zeros(shape, np.float32), f, "all background")
    assert n == 0 and not bool(got.any())
    r, c = np.mgrid[0:rows, 0:cols]
    got, n = _check_label(((r + c) % 2 == 0).astype(np.float32), f, "checkerboard")
    assert n == 1
    got, n = _check_label(((r % 2 == 0) & (c % 2 == 0)).astype(np.float32), f, "isolated pixels")
    assert n == ((rows + 1) // 2) * ((cols + 1) // 2)


def test_label_serpentine_and_spiral():
    got, n = _check_label((serpentine() > 0).astype(np.float32), what="serpentine")
    assert n == 1
    sp = double_spiral()
    got, n = _check_label(sp, what="double spiral")
    assert n == 2


def test_label_diagonals_through_tile_corners():
    """one-pixel diagonals laid exactly through tile corners, every (dx, dy) crossing"""
    rows, cols = 3 * TILE_H + 5, 3 * TILE_W + 7
    f = _handle((rows, cols))
    for cy in (TILE_H, 2 * TILE_H, 3 * TILE_H):
        for cx in (TILE_W, 2 * TILE_W, 3 * TILE_W):
            for dx, dy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
                # from the pixel that touches the corner (cy, cx) in quadrant (-dx, -dy) into the one in quadrant (dx, dy), and on
                y0, x0 = cy - (1 if dy > 0 else 0), cx - (1 if dx > 0 else 0)
                m = np.zeros((rows, cols), np.float32)
                for t in range(-3, 5):
                    m[y0 + t * dy, x0 + t * dx] = 1
                m[0, 0] = 1   # and something else
                got, n = _check_label(m, f)
                assert n == 2
    # full-length diagonals and anti-diagonals through every corner at once
    r, c = np.mgrid[0:rows, 0:cols]
    for m in ((r * TILE_W == c * TILE_H), (r % TILE_H == c % TILE_W), ((r + c) % TILE_H == TILE_H - 1), (r - c == 0), (r + c == cols - 1)):
        _check_label(m.astype(np.float32), f, "diagonal family")


@pytest.mark.parametrize("kind", ["g2", "g4"])
def test_mask_kinds_memory_and_pitch(kind):
    rows, cols = 150, 203
    f = _handle((rows, cols), kind)
    rng = np.random.default_rng(3)
    m = _random_mask((rows, cols), 0.4, seed=5)
    # f32 masks with NaN / -1 / +inf sprinkled
    v = m * rng.random((rows, cols), dtype=np.float32)
    v.flat[rng.integers(0, v.size, 300)] = np.nan
    v.flat[rng.integers(0, v.size, 300)] = -1.0
    v.flat[rng.integers(0, v.size, 300)] = np.inf
    want, wn = M.label(v)
    got, n = f.label(torch.from_numpy(v).to(DEV))
    assert n == wn and np.array_equal(got.cpu().numpy(), want)
    # host planes equal device planes
    hgot, hn = f.label(v)
    assert isinstance(hgot, np.ndarray) and hgot.dtype == np.int32 and hn == wn and np.array_equal(hgot, want)
    # u8 masks, device and host
    b = np.where(M.foreground(v), rng.integers(1, 256, v.shape), 0).astype(np.uint8)
    got, n = f.label(torch.from_numpy(b).to(DEV))
    assert n == wn and np.array_equal(got.cpu().numpy(), want)
    hgot, hn = f.label(b)
    assert hn == wn and np.array_equal(hgot, want)
    # pitched inputs and outputs: column windows of wider buffers
    wide_in = torch.full((rows, cols + 9), float("nan"), device=DEV)
    wide_in[:, 3:3 + cols] = torch.from_numpy(v).to(DEV)
    wide_out = torch.full((rows, cols + 5), -7, dtype=torch.int32, device=DEV)
    got, n = f.label(wide_in[:, 3:3 + cols], out=wide_out[:, 1:1 + cols])
    assert n == wn and np.array_equal(wide_out[:, 1:1 + cols].cpu().numpy(), want)
    assert bool((wide_out[:, 0] == -7).all()) and bool((wide_out[:, 1 + cols:] == -7).all())
    wide_b = torch.zeros((rows, cols + 11), dtype=torch.uint8, device=DEV)
    wide_b[:, 2:2 + cols] = torch.from_numpy(b).to(DEV)
    got, n = f.label(wide_b[:, 2:2 + cols])
    assert n == wn and np.array_equal(got.cpu().numpy(), want)
    hwide = np.full((rows, cols + 4), -7, np.int32)
    f.label(np.ascontiguousarray(v), out=hwide[:, 2:2 + cols])
    assert np.array_equal(hwide[:, 2:2 + cols], want) and (hwide[:, :2] == -7).all() and (hwide[:, 2 + cols:] == -7).all()
    # a non-default stream
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, n = f.label(torch.from_numpy(v).to(DEV))
    s.synchronize()
    assert n == wn and np.array_equal(got.cpu().numpy(), want)
    torch.cuda.synchronize()
    f.label(torch.from_numpy(v).to(DEV))   # back on the default stream


def test_label_run_to_run_identity():
    m = torch.from_numpy(_random_mask((517, 731), 0.45)).to(DEV)
    f = _handle((517, 731))
    first, n0 = f.label(m)
    for _ in range(9):
        again, n = f.label(m)
        assert n == n0 and torch.equal(again, first)


def _bits(t):
    return np.ascontiguousarray(t["peak"]).view(np.uint32)


def _check_table(got, want):
    for name in M.COMPONENT_DTYPE.names[:-1]:
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("shape", [(3, 257), (517, 731), (1080, 1920)])
def test_component_stats(shape):
    rng = np.random.default_rng(11)
    m = _random_mask(shape, 0.45, seed=shape[0])
    f = _handle(shape)
    lab, n = f.label(torch.from_numpy(m).to(DEV))
    w = (rng.integers(-3, 6, shape) * 0.5).astype(np.float32)      # few distinct values: repeated maxima everywhere
    w.flat[rng.integers(0, w.size, w.size // 20 + 1)] = np.nan
    w.flat[rng.integers(0, w.size, w.size // 20 + 1)] = -0.0
    w.flat[rng.integers(0, w.size, w.size // 20 + 1)] = 0.0
    hl = lab.cpu().numpy()
    want = M.stats(hl, n, w)
    _check_table(f.component_stats(lab, n, torch.from_numpy(w).to(DEV)), want)
    _check_table(f.component_stats(hl, n, w), want)                                   # host planes
    _check_table(f.component_stats(lab, n), M.stats(hl, n))                           # no weight: no peak
    # a device table
    table = torch.zeros((max(n, 1), 10), dtype=torch.int32, device=DEV)
    pl, pw = cv.api._plane(lab), cv.api._plane(torch.from_numpy(w).to(DEV))
    rc = L.lib().cvs_component_stats(f._h, C.byref(pl), n, C.byref(pw), C.c_void_p(table.data_ptr()), L.MEM_DEVICE)
    assert rc == 0
    _check_table(table.cpu().numpy()[:n].copy().view(M.COMPONENT_DTYPE).reshape(-1), want)
    # out-of-range labels leave the table to the in-range pixels
    bad = hl.copy()
    bad.flat[rng.integers(0, bad.size, 50)] = n + 1
    bad.flat[rng.integers(0, bad.size, 50)] = -3
    bad.flat[rng.integers(0, bad.size, 50)] = 2 ** 31 - 1
    half = max(1, n // 2)
    _check_table(f.component_stats(torch.from_numpy(bad).to(DEV), half, torch.from_numpy(w).to(DEV)), M.stats(bad, half, w))
    assert len(f.component_stats(lab, 0)) == 0


@pytest.mark.parametrize("shape", [(2, 2), (517, 731)])
def test_prune_random(shape):
    rng = np.random.default_rng(5)
    f = _handle(shape)
    masks = [_random_mask(shape, d, seed=9 + i) for i, d in enumerate((0.3, 0.2, 0.45))]
    ws = [rng.random(shape, dtype=np.float32) * masks[i] for i in range(3)]
    ws[1].flat[rng.integers(0, ws[1].size, ws[1].size // 10 + 1)] = np.nan
    dm = [torch.from_numpy(m).to(DEV) for m in masks]
    dw = [torch.from_numpy(w).to(DEV) for w in ws]
    for min_area in (0, 1, 2, 8, 10 ** 9):
        for dtype in (torch.uint8, torch.float32):
            # n = 1 and 3, without weight
            got, kept = f.prune(dm, min_area, dtype=dtype, return_kept=True)
            for g, k, m in zip(got, kept, masks):
                want, wk = M.prune(m, min_area)
                assert g.dtype == dtype and k == wk
                assert np.array_equal(g.cpu().numpy().astype(np.uint8), want) and set(np.unique(g.cpu().numpy()).tolist()) <= {0, 255}
            g1, k1 = f.prune(dm[0], min_area, dtype=dtype, return_kept=True)
            assert torch.equal(g1, got[0]) and k1 == kept[0]
        for min_peak in (0.0, 0.5, 0.9, 0.999, -float("inf"), float("inf")):
            got, kept = f.prune(dm, min_area, weight=dw, min_peak=min_peak, return_kept=True)
            for g, k, m, w in zip(got, kept, masks, ws):
                want, wk = M.prune(m, min_area, w, min_peak)
                assert k == wk and np.array_equal(g.cpu().numpy(), want)
    # min_area = 0 without weight reproduces the mask's foreground
    assert np.array_equal(f.prune(dm[0], 0).cpu().numpy() == 255, masks[0] > 0)
    # host planes, u8 masks
    hg, hk = f.prune(masks[0], 8, weight=ws[0], min_peak=0.9, return_kept=True)
    want, wk = M.prune(masks[0], 8, ws[0], 0.9)
    assert isinstance(hg, np.ndarray) and hg.dtype == np.uint8 and hk == wk and np.array_equal(hg, want)
    hf = f.prune(masks[0], 8, dtype=np.float32)
    assert hf.dtype == np.float32 and np.array_equal(hf.astype(np.uint8), M.prune(masks[0], 8)[0])
    b = (masks[2] * 255).astype(np.uint8)
    assert np.array_equal(f.prune(torch.from_numpy(b).to(DEV), 8).cpu().numpy(), M.prune(b, 8)[0])
    assert np.array_equal(f.prune(b, 8), M.prune(b, 8)[0])


def test_prune_thinned_fish_and_contours(fish):
    img = torch.from_numpy(fish).to(DEV)
    f = cv.SteerableFiltersG2(img)
    thin = f.nonmax(f.pipeline(img)[5:8])
    hi = float(max(float(t.max()) for t in thin))
    low, high = 0.05 * hi, 0.2 * hi
    masks = f.hysteresis(list(thin), low, high)
    for min_area, min_peak in ((0, 0.0), (8, 0.0), (2, 0.5 * hi), (30, 0.3 * hi)):
        got, kept = f.prune(masks, min_area, weight=thin, min_peak=min_peak, return_kept=True)
        for g, k, m, t in zip(got, kept, masks, thin):
            want, wk = M.prune(m.cpu().numpy(), min_area, t.cpu().numpy(), min_peak)
            assert k == wk and np.array_equal(g.cpu().numpy(), want)
    # contours(): unchanged by default; with min_area the prune of it
    plain = f.contours(img, 20.0, 60.0)
    maps = f.pipeline(img)
    t2 = f.nonmax(maps[5:8])
    want = f.hysteresis(t2, 20.0, 60.0)
    assert len(plain) == 3 and all(torch.equal(a, b) and a.dtype == torch.uint8 for a, b in zip(plain, want))
    pruned = f.contours(img, 20.0, 60.0, min_area=6)
    for a, b in zip(pruned, f.prune(want, 6, weight=t2)):
        assert torch.equal(a, b)
    assert all(bool((a <= b).all()) for a, b in zip(pruned, plain))


@pytest.mark.parametrize("shape", [(1, 37), (517, 731), (1080, 1920)])
def test_contour_points(shape):
    f = _handle(shape)
    m = _random_mask(shape, 0.3, seed=shape[1])
    lab, n = f.label(torch.from_numpy(m).to(DEV))
    hl = lab.cpu().numpy()
    want = M.points(hl)
    got = f.contour_points(lab)
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(f.contour_points(hl), want)                      # host
    wide = torch.zeros((shape[0], shape[1] + 6), dtype=torch.int32, device=DEV)
    wide[:, 4:4 + shape[1]] = lab
    assert np.array_equal(f.contour_points(wide[:, 4:4 + shape[1]]).cpu().numpy(), want)
    # capacity one short: CVS_E_SIZE, n_points set, the buffer untouched
    npts = len(want)
    buf = torch.full((npts, 3), -9, dtype=torch.int32, device=DEV)
    cnt = C.c_int(-1)
    pl = cv.api._plane(lab)
    rc = L.lib().cvs_contour_points(f._h, C.byref(pl), C.c_void_p(buf.data_ptr()), npts - 1, L.MEM_DEVICE, C.byref(cnt))
    torch.cuda.synchronize()
    assert rc == L.E_SIZE and cnt.value == npts and bool((buf == -9).all())
    rc = L.lib().cvs_contour_points(f._h, C.byref(pl), C.c_void_p(buf.data_ptr()), npts, L.MEM_DEVICE, C.byref(cnt))
    assert rc == 0 and np.array_equal(buf.cpu().numpy(), want)
    # grouped: offsets agree with the table's areas, every group in raster order
    pts, off = f.contour_points(lab, group=True)
    table = f.component_stats(lab, n)
    p, o = pts.cpu().numpy(), off.cpu().numpy()
    assert len(o) == n + 1 and np.array_equal(np.diff(o), table["area"])
    for k in (1, n // 2 + 1, n):
        seg = p[o[k - 1]:o[k]]
        assert (seg[:, 2] == k).all() and np.array_equal(seg, want[want[:, 2] == k])
        assert (seg[0, 0], seg[0, 1]) == (table["first_x"][k - 1], table["first_y"][k - 1])
    hp, ho = f.contour_points(hl, group=True)
    assert np.array_equal(hp, p) and np.array_equal(ho, o)
    # nothing labelled
    empty = f.contour_points(torch.zeros(shape, dtype=torch.int32, device=DEV))
    assert tuple(empty.shape) == (0, 3)


# ---- errors: a code each, and nothing written ----
def test_errors():
    rows, cols = 64, 96
    f = _handle((rows, cols))
    lib = L.lib()
    pl = lambda ts: (L.Plane * len(ts))(*[cv.api._plane(t) for t in ts])
    one = lambda t: C.byref(cv.api._plane(t))
    mask = (torch.rand(rows, cols, device=DEV) < 0.4).float()
    w = torch.rand(rows, cols, device=DEV)
    lab = torch.full((rows, cols), 7, dtype=torch.int32, device=DEV)
    outs = [torch.full((rows, cols), 7, dtype=torch.uint8, device=DEV) for _ in range(3)]
    fout = torch.full((rows, cols), 7.0, device=DEV)
    small = torch.rand(rows - 1, cols, device=DEV)
    small_lab = torch.zeros((rows - 1, cols), dtype=torch.int32, device=DEV)
    n = C.c_int(-1)
    kept = (C.c_int * 3)(-1, -1, -1)
    # cvs_label
    assert lib.cvs_label(f._h, one(mask), one(fout), C.byref(n)) == L.E_BADARG                     # labels not S32
    assert lib.cvs_label(f._h, one(mask), one(outs[0]), C.byref(n)) == L.E_BADARG
    as_lab = cv.api._plane(mask)
    as_lab.mem |= L.DEPTH_S32
    assert lib.cvs_label(f._h, one(mask), C.byref(as_lab), C.byref(n)) == L.E_BADARG               # labels overlaps the mask
    assert lib.cvs_label(f._h, one(small), one(lab), C.byref(n)) == L.E_SIZE
    assert lib.cvs_label(f._h, one(mask), one(small_lab), C.byref(n)) == L.E_SIZE
    assert lib.cvs_label(f._h, None, one(lab), C.byref(n)) == L.E_BADARG
    fresh = cv.SteerableFiltersG2(None)
    assert lib.cvs_label(fresh._h, one(mask), one(lab), C.byref(n)) == L.E_STATE                  # no setup
    assert lib.cvs_contour_prune(fresh._h, 1, pl([mask]), None, 0, 0.0, pl(outs[:1]), kept) == L.E_STATE
    assert lib.cvs_component_stats(fresh._h, one(lab), 1, None, C.c_void_p(lab.data_ptr()), L.MEM_DEVICE) == L.E_STATE
    assert lib.cvs_contour_points(fresh._h, one(lab), None, 0, L.MEM_HOST, C.byref(n)) == L.E_STATE
    # cvs_component_stats
    tab = torch.full((4, 10), 7, dtype=torch.int32, device=DEV)
    assert lib.cvs_component_stats(f._h, one(mask), 4, None, C.c_void_p(tab.data_ptr()), L.MEM_DEVICE) == L.E_BADARG    # labels not S32
    assert lib.cvs_component_stats(f._h, one(lab), -1, None, C.c_void_p(tab.data_ptr()), L.MEM_DEVICE) == L.E_BADARG
    assert lib.cvs_component_stats(f._h, one(lab), 4, None, None, L.MEM_DEVICE) == L.E_BADARG
    assert lib.cvs_component_stats(f._h, one(lab), 4, one(outs[0]), C.c_void_p(tab.data_ptr()), L.MEM_DEVICE) == L.E_BADARG   # u8 weight
    assert lib.cvs_component_stats(f._h, one(small_lab), 4, None, C.c_void_p(tab.data_ptr()), L.MEM_DEVICE) == L.E_SIZE
    assert lib.cvs_component_stats(f._h, one(lab), 4, one(small), C.c_void_p(tab.data_ptr()), L.MEM_DEVICE) == L.E_SIZE
    # cvs_contour_prune
    assert lib.cvs_contour_prune(f._h, 0, pl([mask]), None, 0, 0.0, pl(outs[:1]), kept) == L.E_BADARG
    assert lib.cvs_contour_prune(f._h, 1, pl([mask]), None, -1, 0.0, pl(outs[:1]), kept) == L.E_BADARG
    assert lib.cvs_contour_prune(f._h, 1, pl([mask]), pl([w]), 0, float("nan"), pl(outs[:1]), kept) == L.E_BADARG
    assert lib.cvs_contour_prune(f._h, 2, pl([mask, mask]), None, 0, 0.0, pl([outs[0], fout]), kept) == L.E_BADARG      # mixed depths
    assert lib.cvs_contour_prune(f._h, 1, pl([fout]), None, 0, 0.0, pl([fout]), kept) == L.E_BADARG                     # out is the mask
    assert lib.cvs_contour_prune(f._h, 1, pl([mask]), pl([fout]), 0, 0.0, pl([fout]), kept) == L.E_BADARG               # out is the weight
    assert lib.cvs_contour_prune(f._h, 2, pl([mask, mask]), None, 0, 0.0, pl([outs[1], outs[1]]), kept) == L.E_BADARG   # outputs overlap
    assert lib.cvs_contour_prune(f._h, 1, pl([small]), None, 0, 0.0, pl(outs[:1]), kept) == L.E_SIZE
    assert lib.cvs_contour_prune(f._h, 1, pl([mask]), None, 0, 0.0, None, kept) == L.E_BADARG
    # cvs_contour_points
    assert lib.cvs_contour_points(f._h, one(mask), None, 0, L.MEM_HOST, C.byref(n)) == L.E_BADARG                        # not S32
    assert lib.cvs_contour_points(f._h, one(lab), None, 0, L.MEM_HOST, None) == L.E_BADARG
    assert lib.cvs_contour_points(f._h, one(lab), None, 5, L.MEM_HOST, C.byref(n)) == L.E_BADARG
    assert lib.cvs_contour_points(f._h, one(lab), None, -1, L.MEM_HOST, C.byref(n)) == L.E_BADARG
    assert lib.cvs_contour_points(f._h, one(small_lab), None, 0, L.MEM_HOST, C.byref(n)) == L.E_SIZE
    assert n.value == -1 and list(kept) == [-1, -1, -1]
    torch.cuda.synchronize()
    assert bool((lab == 7).all()) and bool((fout == 7.0).all()) and bool((tab == 7).all()) and all(bool((o == 7).all()) for o in outs)
    # capture: all four refuse
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    good, count = f.label(mask)
    with torch.cuda.stream(side):
        f.label(mask)                           # the handle moves to the side stream outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            fout.fill_(1.0)
            rcs = [lib.cvs_label(f._h, one(mask), one(lab), C.byref(n)),
                   lib.cvs_component_stats(f._h, one(good), 4, None, C.c_void_p(tab.data_ptr()), L.MEM_DEVICE),
                   lib.cvs_contour_prune(f._h, 1, pl([mask]), None, 0, 0.0, pl(outs[:1]), kept),
                   lib.cvs_contour_points(f._h, one(good), None, 0, L.MEM_HOST, C.byref(n))]
    assert rcs == [L.E_UNSUPPORTED] * 4
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert bool((lab == 7).all()) and bool((tab == 7).all()) and bool((outs[0] == 7).all()) and n.value == -1
    again, count2 = f.label(mask)               # and the handle works afterwards
    assert count2 == count and torch.equal(again, good)


def test_facade_members(tmp_path, fish):
    exe = os.path.join(str(tmp_path), "test_components")
    lib = os.path.join(ROOT, "cvsteer_amd")
    if not os.path.exists(os.path.join(lib, "libcvsteer.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cvsteer_amd", "facade"), "-s"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-DCVSTEER_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_components.cpp"), "-L" + lib, "-lcvsteer", "-lcvsteer_hip",
                           "-Wl,-rpath," + lib])
    raw = os.path.join(str(tmp_path), "fish.f32")
    fish.astype(np.float32).tofile(raw)
    r = subprocess.run([exe, raw, str(fish.shape[0]), str(fish.shape[1])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "components OK" in r.stdout


def test_label_time_does_not_depend_on_the_shape_of_the_contour():
    """label of the one-pixel serpentine against hysteresis of the same plane, wall clock around the (synchronising) calls"""
    v = torch.from_numpy(serpentine()).to(DEV)
    f = _handle((1024, 1024))
    f.label(v)
    f.hysteresis(v, 0.25, 0.75)   # warm both: scratch allocated, code loaded
    torch.cuda.synchronize()
    t_label, t_hyst = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        lab, n = f.label(v)
        t1 = time.perf_counter()
        out, passes = f.hysteresis(v, 0.25, 0.75, return_passes=True)
        t2 = time.perf_counter()
        t_label.append(t1 - t0)
        t_hyst.append(t2 - t1)
    assert n == 1 and bool(((out == 255) == (v > 0)).all())
    a, b = float(np.median(t_label)), float(np.median(t_hyst))
    print("serpentine 1024^2: label %.3f ms, hysteresis %.3f ms (%d passes), ratio %.1f" % (1e3 * a, 1e3 * b, passes, b / a))
    assert a < b
